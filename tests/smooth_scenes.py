"""The meshes the mesh-smoothing tests share (test_smooth_cpu.py, test_smooth_gpu.py): cases worked by hand, the strips and soups of
components_scenes, a fan of 70000 triangles around one hub - one row of 140000 slots, one vertex in every edge key - and the field
meshes of components_scenes.  Nothing is copied: the meshes are components_scenes' own.  Everything is numpy and is computed once;
nothing changes a mesh or a result afterwards."""
import numpy as np

from be_hip import smooth
import components_scenes as cs

_F = np.float32
KEYS = ("vertices", "faces", "weight", "feat", "normal", "normal_valid", "edge", "valence", "boundary", "displacement")
ADJACENCY_KEYS = ("valence", "boundary")
NORMAL_KEYS = ("normal", "normal_valid")
NAN, INF = float("nan"), float("inf")
EDGE = 65536.0                                                           # 2^16: the first |x| that is not usable
BELOW_EDGE = float(np.nextafter(_F(EDGE), _F(0)))                         # the last that is

_TRI = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
_TET = [(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4)]
_QUAD = [(0, 0, 0), (4, 0, 0), (0, 4, 0), (4, 4, 0)]
# a hexagon whose corners add up to 0 in X and Y, around a hub lifted by 0.25
_HEX = [(0, 0, 0.25), (2, 0, 0), (1, 2, 0), (-1, 2, 0), (-2, 0, 0), (-1, -2, 0), (1, -2, 0)]
_HEX_FACES = [[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 6], [0, 6, 1]]
_STEP = dict(iters=1, mu=0.0)                                            # one step with lam = 0.5

# name -> (mesh, kw of smooth, the answer worked by hand: valence, boundary and - where given - the new positions, exact)
HAND = {
    "no vertex": (cs.bare(np.zeros((0, 3)), np.zeros((0, 3))), {}, dict(valence=[], boundary=[], vertices=[])),
    "vertices without a face": (cs.bare(_TRI, np.zeros((0, 3))), {}, dict(valence=[0, 0, 0], boundary=[0, 0, 0], vertices=_TRI)),
    "one triangle, fixed": (cs.bare(_TRI, [[0, 1, 2]]), {}, dict(valence=[1, 1, 1], boundary=[1, 1, 1], vertices=_TRI)),
    # a: slots (b, c), S / 2 = (2, 2, 0), d = (2, 2, 0), Q' = (1, 1, 0); b: S / 2 = (0, 2, 0), d = (-4, 2, 0), Q' = (2, 1, 0); c alike
    "one triangle, free, one step": (cs.bare(_TRI, [[0, 1, 2]]), dict(_STEP, boundary="free"),
                                     dict(valence=[1, 1, 1], boundary=[1, 1, 1], vertices=[(1, 1, 0), (2, 1, 0), (1, 2, 0)])),
    # closed: every edge in two faces; vertex 0: each neighbour twice, S / 6 = (4/3, 4/3, 4/3) - not exact, so no positions here
    "a tetrahedron": (cs.bare(_TET, [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]]), {}, dict(valence=[3, 3, 3, 3], boundary=[0, 0, 0, 0])),
    "two triangles on a shared edge": (cs.bare(_QUAD, [[0, 1, 2], [2, 1, 3]]), {}, dict(valence=[1, 2, 2, 1], boundary=[1, 1, 1, 1], vertices=_QUAD)),
    # 1: slots (2, 0), (3, 2): S = (0, 4, 0) + (0, 0, 0) + (4, 4, 0) + (0, 4, 0) = (4, 12, 0), / 4 = (1, 3, 0), d = (-3, 3, 0): (2.5, 1.5, 0)
    # 2: slots (0, 1), (1, 3): S = (0 + 4 + 4 + 4, 0 + 0 + 0 + 4, 0) = (12, 4, 0), / 4 = (3, 1, 0), d = (3, -3, 0): (1.5, 2.5, 0)
    # 0: (1, 2): (2, 2, 0), d = (2, 2, 0): (1, 1, 0);  3: (2, 1): (2, 2, 0), d = (-2, -2, 0): (3, 3, 0)
    "two triangles, free, one step": (cs.bare(_QUAD, [[0, 1, 2], [2, 1, 3]]), dict(_STEP, boundary="free"),
                                      dict(valence=[1, 2, 2, 1], boundary=[1, 1, 1, 1], vertices=[(1, 1, 0), (2.5, 1.5, 0), (1.5, 2.5, 0), (3, 3, 0)])),
    # the hub's 12 slots hold every ring vertex twice: S / 12 = (0, 0, 0), d = (0, 0, -h), Q' = (1 - lam) h exactly; the ring is held
    "a hexagonal fan, one step": (cs.bare(_HEX, _HEX_FACES), _STEP,
                                  dict(valence=[6, 2, 2, 2, 2, 2, 2], boundary=[0, 1, 1, 1, 1, 1, 1], vertices=[(0, 0, 0.125)] + _HEX[1:])),
    "a hexagonal fan, lam 0.25": (cs.bare(_HEX, _HEX_FACES), dict(_STEP, lam=0.25),
                                  dict(valence=[6, 2, 2, 2, 2, 2, 2], boundary=[0, 1, 1, 1, 1, 1, 1], vertices=[(0, 0, 0.1875)] + _HEX[1:])),
    # every edge in two faces: no boundary, and a: S / 4 = (2, 2, 0) as in one triangle - a face given twice counts twice
    "a face given twice": (cs.bare(_TRI, [[0, 1, 2], [0, 1, 2]]), _STEP,
                           dict(valence=[2, 2, 2], boundary=[0, 0, 0], vertices=[(1, 1, 0), (2, 1, 0), (1, 2, 0)])),
    "a repeated index": (cs.bare(_QUAD, [[0, 0, 1], [3, 1, 3], [0, 1, 2]]), dict(_STEP, boundary="free"),
                         dict(valence=[1, 1, 1, 0], boundary=[1, 1, 1, 0], vertices=[(1, 1, 0), (2, 1, 0), (1, 2, 0), (4, 4, 0)])),
    # vertex 3 is not usable and takes face 1 with it: vertices 0, 1, 2 see one triangle; 3 keeps its bits
    "a vertex that is not a number": (cs.bare(_TRI + [(NAN, 1, 1)], [[0, 1, 2], [2, 1, 3]]), dict(_STEP, boundary="free"),
                                      dict(valence=[1, 1, 1, 0], boundary=[1, 1, 1, 0], vertices=[(1, 1, 0), (2, 1, 0), (1, 2, 0), (NAN, 1, 1)])),
    "an infinite vertex": (cs.bare(_TRI + [(1, -INF, 1)], [[0, 1, 2], [2, 1, 3]]), dict(_STEP, boundary="free"),
                           dict(valence=[1, 1, 1, 0], boundary=[1, 1, 1, 0], vertices=[(1, 1, 0), (2, 1, 0), (1, 2, 0), (1, -INF, 1)])),
    # |x| = 2^16 is out, the float32 below it is in: face 1 (with vertex 3) does not count, face 2 (with vertex 4) does
    "the last usable coordinate": (cs.bare(_TRI + [(EDGE, 0, 0), (0, -BELOW_EDGE, 0)], [[0, 1, 2], [2, 1, 3], [0, 4, 1]]), {},
                                   dict(valence=[2, 2, 1, 0, 1], boundary=[1, 1, 1, 0, 1], vertices=_TRI + [(EDGE, 0, 0), (0, -BELOW_EDGE, 0)])),
    "no iteration": (cs.bare(_HEX, _HEX_FACES), dict(iters=0, boundary="free"),
                     dict(valence=[6, 2, 2, 2, 2, 2, 2], boundary=[0, 1, 1, 1, 1, 1, 1], vertices=_HEX)),
    # two Laplacian steps of the hub: 0.25 -> 0.125 -> 0.0625
    "mu = 0, two iterations": (cs.bare(_HEX, _HEX_FACES), dict(iters=2, mu=0.0),
                               dict(valence=[6, 2, 2, 2, 2, 2, 2], boundary=[0, 1, 1, 1, 1, 1, 1], vertices=[(0, 0, 0.0625)] + _HEX[1:])),
    # lam then mu = -0.5 on the hub: 0.25 -> 0.125 -> 0.125 - 0.5 * (0 - 0.125) = 0.1875
    "lam and mu, one iteration": (cs.bare(_HEX, _HEX_FACES), dict(iters=1, mu=-0.5),
                                  dict(valence=[6, 2, 2, 2, 2, 2, 2], boundary=[0, 1, 1, 1, 1, 1, 1], vertices=[(0, 0, 0.1875)] + _HEX[1:])),
}
# faces 1 and 2 name what is not there: the statement refuses them, the kernels ignore them
OUT_OF_RANGE = cs.bare(_QUAD, [[0, 1, 2], [0, 1, 4], [3, -1, 2], [2, 1, 3]])
OUT_OF_RANGE_FACES = (1, 2)

FAN = 70000                                                             # triangles around one hub


def fan():
    """FAN triangles (0, i, i + 1) around the hub 0, closed: the ring 1..FAN on a circle of radius 1 that wobbles in Z, the hub
    lifted by 0.3.  The hub's row holds 2 FAN slots, every spoke is an edge key with vertex 0 in it, every ring vertex is boundary
    and the hub is not."""
    def make():
        i = np.arange(FAN)
        t = 2 * np.pi * i / FAN
        ring = np.stack([np.cos(t), np.sin(t), 0.01 * np.sin(40 * t)], 1)
        pos = np.concatenate([[(0.003, -0.002, 0.3)], ring])
        faces = np.stack([np.zeros(FAN, np.int64), 1 + i, 1 + (i + 1) % FAN], 1)
        return cs.bare(pos, faces)
    return cs._once("fan", make)


SYNTHETIC = ["strip ascending 1", "strip descending 1", "strip permuted 1", "fan", "soup", "soup joined"]
CONFIGS = [dict(iters=i, boundary=b, mu=mu) for i in (1, 10) for b in ("fixed", "free") for mu in (-0.53, 0.0)]
FIELD_CONFIGS = [dict(), dict(boundary="free", normals="recompute")]


def get(name):
    if name in HAND:
        return HAND[name][0]
    return fan() if name == "fan" else cs.get(name)


def _key(kw):
    return tuple(sorted(kw.items()))


def ref(name, **kw):
    """smooth.smooth of a named mesh, once per set of arguments (a hand case: on top of its own)."""
    if name in HAND:
        kw = dict(HAND[name][1], **kw)
    return cs._once(("smoothed", name, _key(kw)), lambda: smooth.smooth(get(name), **kw))


def adjacency(name):
    return cs._once(("adjacency", name), lambda: smooth.adjacency(get(name)))


def normals(name):
    return cs._once(("vertex normals", name), lambda: smooth.vertex_normals(get(name)))


ALL = list(HAND) + SYNTHETIC + list(cs.FIELD_NAMES)
