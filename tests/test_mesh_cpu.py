"""The numpy statement of mesh extraction (be_hip/mesh.py) tied to other statements of the same thing: a cell worked by hand, the
properties of the derived case table, an ellipsoid that must come out as a closed oriented surface of the right volume, the
structure of the outputs on a volume with holes, an exact zero on a lattice plane, the plane of test_tsdf_cpu.py, the same
function in float64, and the quality of the fusion scene's mesh beside its ray cast's.  No GPU: the kernels are held to
mesh.extract bit for bit by test_mesh_gpu.py."""
import os

import numpy as np
import pytest

from be_hip import camera, mesh
import mesh_scenes as ms

_F = np.float32


def _extract(f, **kw):
    return mesh.extract(f["D"], f["W"], f["Fm"], f["origin"], f["voxel"], **kw)


def _face_normals(m):
    v, f = m["vertices"].astype(np.float64), m["faces"]
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


# ------------------------------------------------------------------------------------------ 1. a cell worked by hand
def test_hand_worked_cell():
    """A 2 x 2 x 2 volume, origin (0, 0, 0), voxel (1, 2, 4), every voxel observed.  Corner k = 4 dz + 2 dy + dx holds
      D[0] = 0.5 (the one positive corner), D[1] = -0.5, D[2] = -1.5, D[3] = -0.5, D[4] = -0.125, D[5] = -0.5, D[6] = -0.5, D[7] = -1.5.
    The 7 edges that leave voxel 0 are the crossed ones, all owned by voxel 0: edge = 0 .. 6, t = Da / (Da - Db) =
      e0 (1,0,0): 0.5 / 1 = 0.5;  e1 (0,1,0): 0.5 / 2 = 0.25;  e2 (0,0,1): 0.5 / 0.625 = 0.8;  e3 (1,1,0): 0.5;  e4 (1,0,1): 0.5;
      e5 (0,1,1): 0.5;  e6 (1,1,1): 0.5 / 2 = 0.25
    and the positions t * offset * voxel: (0.5, 0, 0), (0, 0.5, 0), (0, 0, 3.2), (0.5, 1, 0), (0.5, 0, 2), (0, 1, 2), (0.25, 0.5, 1).
    Every tetrahedron has p0 = corner 0 positive alone, code 1: one triangle each, over the edges from p0 to p1, p2, p3, which are
    (corners 1, 3), (1, 5), (2, 3), (2, 6), (4, 5), (4, 6) and 7: vertices {0,3,6}, {0,4,6}, {1,3,6}, {1,5,6}, {2,4,6}, {2,5,6}.
    Winding of t = 0 (axes x, y, z): midpoints m0 = (.5, 0, 0), m1 = (.5, .5, 0), m2 = (.5, .5, .5); (m1 - m0) x (m2 - m0) =
    (0, .5, 0) x (0, .5, .5) = (.25, 0, 0); towards the positive corner is -(1, 2/3, 1/3): the dot product is < 0, the last two
    swap: (0, 6, 3).  Weights: W = 1 + k / 8 at corner k, so vertex e0 holds 1 + 0.5 * 0.125 = 1.0625."""
    D = np.array([0.5, -0.5, -1.5, -0.5, -0.125, -0.5, -0.5, -1.5], _F).reshape(2, 2, 2)
    W = (1 + np.arange(8) / 8).astype(_F).reshape(2, 2, 2)
    m = mesh.extract(D, W, None, (0, 0, 0), (1, 2, 4))
    assert m["edge"].dtype == np.int64 and m["edge"].tolist() == [0, 1, 2, 3, 4, 5, 6]
    want = np.array([(0.5, 0, 0), (0, 0.5, 0), (0, 0, 3.2), (0.5, 1, 0), (0.5, 0, 2), (0, 1, 2), (0.25, 0.5, 1)], _F)
    assert m["vertices"].dtype == _F and np.array_equal(m["vertices"], want)
    assert m["weight"][0] == _F(1.0625) and m["weight"][6] == _F(1 + 0.25 * 0.875) and m["feat"] is None
    assert m["faces"].dtype == np.int32 and m["faces"].shape == (6, 3)
    assert [sorted(f) for f in m["faces"].tolist()] == [[0, 3, 6], [0, 4, 6], [1, 3, 6], [1, 5, 6], [2, 4, 6], [2, 5, 6]]
    assert m["faces"][0].tolist() == [0, 6, 3]
    # every winding normal points at the positive corner, the origin; the gradient normals likewise
    n = _face_normals(m)
    centre = m["vertices"][m["faces"]].astype(np.float64).mean(1)
    assert (np.einsum("ij,ij->i", n, -centre) > 0).all()
    assert m["normal_valid"].all() and (np.einsum("ij,ij->i", m["normal"].astype(np.float64), -m["vertices"].astype(np.float64)) > 0).all()
    # the complement: the same vertices, every triangle reversed
    r = mesh.extract(-D, W, None, (0, 0, 0), (1, 2, 4))
    assert np.array_equal(r["vertices"], m["vertices"]) and np.array_equal(r["faces"], m["faces"][:, [0, 2, 1]])


# ------------------------------------------------------------------------------------------ 2. the table
def test_the_case_table():
    tb = mesh.tables()
    assert tb["corners"].tolist() == [[0, 1, 3, 7], [0, 1, 5, 7], [0, 2, 3, 7], [0, 2, 6, 7], [0, 4, 5, 7], [0, 4, 6, 7]]
    for t in range(6):
        for code in range(16):
            bits = bin(code).count("1")
            assert tb["count"][t, code] == {0: 0, 4: 0, 1: 1, 3: 1, 2: 2}[bits]
            tris = tb["pairs"][t, code, :tb["count"][t, code]]
            assert (tb["pairs"][t, code, tb["count"][t, code]:] == -1).all()
            for tri in tris:
                assert all((code >> i & 1) != (code >> j & 1) and i < j for i, j in tri)     # every vertex on a crossed edge
                assert len({tuple(p) for p in tri.tolist()}) == 3
            # the complement covers the same patch - one triangle, or the same quad - with every winding reversed: the area vectors
            # of the midpoint triangles each point at the positive corners, and their sums are opposite
            if tris.size:
                P = np.array([[(k >> ax) & 1 for ax in range(3)] for k in tb["corners"][t]], float)
                pos, neg = [i for i in range(4) if code >> i & 1], [i for i in range(4) if not code >> i & 1]
                towards = P[pos].mean(0) - P[neg].mean(0)
                mid = lambda tr: (P[tr[:, :, 0]] + P[tr[:, :, 1]]) / 2
                area = lambda m: np.cross(m[:, 1] - m[:, 0], m[:, 2] - m[:, 0])
                other = tb["pairs"][t, 15 - code, :tb["count"][t, code]]
                assert (area(mid(tris)) @ towards > 0).all() and (area(mid(other)) @ towards < 0).all()
                assert np.allclose(area(mid(tris)).sum(0), -area(mid(other)).sum(0))
                assert {tuple(p) for p in tris.reshape(-1, 2).tolist()} == {tuple(p) for p in other.reshape(-1, 2).tolist()}
                if len(tris) == 1:
                    assert np.array_equal(other, tris[:, [0, 2, 1]])
    assert tb["cube_count"][0] == 0 and tb["cube_count"][255] == 0 and tb["cube_count"].max() == 12
    assert tb["cube_count"][1] == 6 and tb["cube_count"][2] == 2          # corner 000 lies in all six tetrahedra, corner 100 in two
    assert (tb["cube_count"] == tb["cube_count"][::-1]).all()


def test_the_committed_table_header_is_the_derived_one():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(mesh.__file__))), "csrc", "be_tsdf_mesh_table.h")
    with open(path) as fh:
        assert fh.read() == mesh.table_header()


# ------------------------------------------------------------------------------------------ 3. a closed oriented surface
def _directed_edges(f):
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def test_the_ellipsoid_is_a_closed_oriented_surface():
    """Every undirected edge in exactly two triangles, once per direction; Euler characteristic 2; no triangle repeats an index;
    the normals point towards D > 0, the outside, so the signed volume is positive: 295.4 lattice units against
    4/3 pi 4.2^3 / sqrt(1.3 * 0.8) = 304.3 (a polyhedron inscribed in a convex body).  The CPU prototype of this rule: 1972 triangles, 988 vertices, 295.4."""
    m = ms.reference("ellipsoid", ms.ellipsoid())
    v, f = m["vertices"].astype(np.float64), m["faces"]
    T, V = len(f), len(v)
    assert (T, V) == (1972, 988)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 0] != f[:, 2]).all()
    d = _directed_edges(f)
    key = d[:, 0].astype(np.int64) * V + d[:, 1]
    assert len(np.unique(key)) == len(key)                               # no directed edge twice
    assert np.array_equal(np.sort(key), np.sort(d[:, 1].astype(np.int64) * V + d[:, 0]))      # and each one's reverse is there
    E = len(key) // 2
    assert V - E + T == 2
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6)
    exact = 4 / 3 * np.pi * 4.2 ** 3 / np.sqrt(1.3 * 0.8)
    print(f"ellipsoid: {T} triangles, {V} vertices, signed volume {vol:.2f} against {exact:.2f}")
    assert vol > 0 and abs(vol - exact) <= 0.05 * exact
    assert abs(vol - 295.4) < 0.05
    n = _face_normals(m)
    solid = np.linalg.norm(n, axis=1) > 1e-9
    assert m["normal_valid"].all()
    dots = np.einsum("tkj,tj->tk", m["normal"][f].astype(np.float64), n)
    assert (dots[solid] > 0).all()


# ------------------------------------------------------------------------------------------ 4. structure with holes
def _cells_of(m, dims):
    """The cell of every triangle: the least corner over the endpoints of its three edges (every triangle's edges touch p0)."""
    Nz, Ny, Nx = dims
    owner, e = m["edge"] // 7, m["edge"] % 7
    lo = np.stack([owner % Nx, owner // Nx % Ny, owner // (Nx * Ny)], 1)
    lo = lo[m["faces"]].min(1)
    return (lo[:, 2] * Ny + lo[:, 1]) * Nx + lo[:, 0]


@pytest.mark.parametrize("holes", [False, True])
def test_structure_on_the_planted_volume(holes):
    f = ms.planted(holes)
    m = ms.reference(("planted", holes), f)
    V, T = len(m["vertices"]), len(m["faces"])
    assert V > 500 and T > 500
    assert m["faces"].min() >= 0 and m["faces"].max() < V
    assert len(np.unique(m["faces"])) == V                               # every vertex is referenced
    assert (np.diff(m["edge"]) > 0).all()
    cells = _cells_of(m, f["D"].shape)
    assert (np.diff(cells) >= 0).all()
    Nz, Ny, Nx = f["D"].shape
    Wf = f["W"].reshape(-1)
    for k in range(8):
        assert (Wf[cells + ((k >> 2 & 1) * Ny + (k >> 1 & 1)) * Nx + (k & 1)] > 0).all()
    if not holes:
        # the cell at ix = 2c has cube code c: its triangle count is the table's
        counts = np.bincount(cells, minlength=Nx)[:Nx:2]
        assert np.array_equal(counts, mesh.tables()["cube_count"])
        seen = {(t, sum((c >> int(mesh.tables()["corners"][t, i]) & 1) << i for i in range(4))) for c in range(256) for t in range(6)}
        assert len(seen) == 96                                           # every tet case occurs
    else:
        assert T < len(ms.reference(("planted", False), ms.planted(False))["faces"])
    for k in ("vertices", "weight", "feat", "normal"):
        assert np.isfinite(m[k]).all(), k
    assert m["feat"].shape == (2, V) and m["normal"].shape == (V, 3) and m["normal_valid"].dtype == np.bool_


# ------------------------------------------------------------------------------------------ 5. an exact zero on a lattice plane
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_an_exact_zero_on_a_lattice_plane(sign):
    """D = +-(z - 3): exactly 0 on the layer z = 3, which is not positive.  Every crossed edge has one end on that layer, so t is 0
    (the owner lies on it) or 1 and every vertex sits on a voxel centre of z = 3; the triangles between coinciding vertices have
    no area and stay."""
    z = np.arange(5.0)[:, None, None] * np.ones((5, 6, 7))
    m = mesh.extract(sign * (z - 3), np.ones_like(z))
    assert len(m["faces"]) > 0
    for k in ("vertices", "weight", "normal"):
        assert np.isfinite(m[k]).all(), k
    assert (m["vertices"][:, 2] == 3).all()
    assert np.array_equal(m["vertices"], np.round(m["vertices"]))         # t in {0, 1}: lattice points
    owner_z = m["edge"] // 7 // 42
    assert set(owner_z.tolist()) == ({3} if sign > 0 else {2})            # t = 0: the owner is on the zero layer; t = 1: the far end is
    assert m["normal_valid"].all() and (np.sign(m["normal"][:, 2]) == sign).all()
    area = np.linalg.norm(_face_normals(m), axis=1)
    assert (area == 0).any() and (area > 0).any()


# ------------------------------------------------------------------------------------------ 6. the plane
def test_the_plane_is_recovered():
    """One identity view of the plane Z = 0.9137: the signed distance is linear in z and constant across x and y, so the
    interpolation along an edge is exact; what is left is two dq values each off by at most half of trunc / 32768 = 0.76e-6 m and
    a few float32 ulps at 1 m - the bound of test_tsdf_cpu.py's plane, for the same reason."""
    m = ms.reference("plane", ms.plane())
    assert len(m["vertices"]) > 1000
    err = np.abs(m["vertices"][:, 2].astype(np.float64) - float(_F(ms.PLANE_Z)))
    print(f"plane: {len(m['vertices'])} vertices, {len(m['faces'])} triangles, worst error {err.max():.3e} m")
    assert err.max() <= 1e-5
    assert (m["normal"][m["normal_valid"]][:, 2] < -0.99).all()           # D > 0 in front of the plane: towards the camera


# ------------------------------------------------------------------------------------------ 7. float32 against float64
def test_float32_against_float64():
    """Positivity is decided on D, float32 in both evaluations: topology, faces and edge are identical.  Positions: t is one
    division of a float32 difference, the lerp two more roundings at magnitudes of 1 m - a few ulps of 6e-8: 2e-6 m, the ray
    cast's bound for the same formula.  Measured: profiles/HISTORY.md."""
    f = ms.prototype(8)
    a, b = ms.reference("prototype8", f), ms.reference("prototype8", f, dtype=np.float64)
    assert np.array_equal(a["faces"], b["faces"]) and np.array_equal(a["edge"], b["edge"])
    worst = float(np.abs(a["vertices"].astype(np.float64) - b["vertices"]).max())
    both = a["normal_valid"] & b["normal_valid"]
    nworst = float(np.abs(a["normal"][both].astype(np.float64) - b["normal"][both]).max())
    print(f"float32 / float64: {len(a['vertices'])} vertices, positions differ by at most {worst:.3e} m, weights by "
          f"{float(np.abs(a['weight'].astype(np.float64) - b['weight']).max()):.3e}, normals by {nworst:.3e}, "
          f"normal_valid differs on {int((a['normal_valid'] != b['normal_valid']).sum())}")
    assert len(a["vertices"]) > 1000 and worst <= 2e-6


# ------------------------------------------------------------------------------------------ 8. quality
def test_quality_on_the_fusion_scene():
    """mesh_scenes.quality on the mesh of the prototype's volume at 1 / 5 / 8 views, beside the ray cast's 0.62 / 0.38 / 0.31 cm: no
    vertex off both surfaces, RMSE under the scene's noise of 1 cm and falling with the views.  Figures: profiles/HISTORY.md."""
    q = {V: ms.quality(ms.reference(("prototype", V), ms.prototype(V))) for V in (1, 5, 8)}
    for V in (1, 5, 8):
        print(f"V = {V}: {q[V]['vertices']} vertices scored, rmse {100 * q[V]['rmse']:.3f} cm, wrong {q[V]['wrong']}")
    for V in (1, 5, 8):
        assert q[V]["vertices"] > 500 and q[V]["wrong"] == 0
        assert q[V]["rmse"] < 0.01
    assert q[1]["rmse"] > q[5]["rmse"] > q[8]["rmse"]


# ------------------------------------------------------------------------------------------ 9. smaller checks
def test_raising_min_weight_only_removes():
    f = ms.scene_field(ms.BIG, 3)
    sets = [set(_extract(f, min_weight=w, normals=False)["edge"].tolist()) for w in (0.0, 0.5, 1.5, 4.0)]
    assert len(sets[0]) > len(sets[2]) > 0
    for a, b in zip(sets, sets[1:]):
        assert b <= a


@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("colour", [True, False])
def test_ply_round_trip(tmp_path, normals, colour):
    f = ms.planted(True)
    for m in (_extract(f, normals=normals), _extract(dict(f, W=np.zeros_like(f["W"])), normals=normals)):
        V = len(m["vertices"])
        c = np.linspace(-0.2, 1.2, 3 * V, dtype=_F).reshape(3, V) if colour else None
        path = str(tmp_path / f"m{V}.ply")
        mesh.write_ply(path, m, colour=c)
        back = mesh.read_ply(path)
        assert back["vertices"].dtype == _F and np.array_equal(back["vertices"].view(np.uint32), m["vertices"].view(np.uint32))
        assert back["faces"].dtype == np.int32 and np.array_equal(back["faces"], m["faces"])
        if normals:
            assert np.array_equal(back["normal"].view(np.uint32), np.ascontiguousarray(m["normal"]).view(np.uint32))
        else:
            assert back["normal"] is None
        if colour:
            want = np.floor(np.clip(c, 0, 1) * _F(255) + _F(0.5)).astype(np.uint8)
            assert back["colour"].dtype == np.uint8 and np.array_equal(back["colour"], want)
            if V:
                assert want.min() == 0 and want.max() == 255
        else:
            assert back["colour"] is None
    assert V == 0 and back["vertices"].shape == (0, 3) and back["faces"].shape == (0, 3)
    with open(path, "rb") as fh:
        assert fh.read().startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\n")


def test_check_totals_and_empty_results():
    assert mesh.check_totals(0, 0) == (0, 0) and mesh.check_totals(2 ** 31 - 1, 5) == (2 ** 31 - 1, 5)
    for V, T in ((2 ** 31, 0), (0, 2 ** 31), (-1, 0), (2 ** 40, 2 ** 40)):
        with pytest.raises(ValueError):
            mesh.check_totals(V, T)
    for dims in ((1, 1, 1), (1, 5, 5), (2, 2, 2)):
        m = mesh.extract(np.ones(dims, _F), np.ones(dims, _F), np.ones((2,) + dims, _F))
        assert m["vertices"].shape == (0, 3) and m["vertices"].dtype == _F and m["faces"].shape == (0, 3) and m["faces"].dtype == np.int32
        assert m["weight"].shape == (0,) and m["feat"].shape == (2, 0) and m["normal"].shape == (0, 3) and m["normal_valid"].shape == (0,)
        assert m["edge"].shape == (0,) and m["edge"].dtype == np.int64
    # a single layer has no cell, whatever it holds
    assert len(mesh.extract(np.array([[[1, -1, 1, -1, 1]] * 5], _F), np.ones((1, 5, 5), _F))["faces"]) == 0
    m = mesh.extract(np.ones((3, 3, 3), _F), np.ones((3, 3, 3), _F), normals=False)
    assert m["normal"] is None and m["normal_valid"] is None and m["feat"] is None


def test_rejected_inputs():
    D = W = np.ones((3, 4, 5), _F)
    mesh.extract(D, W)
    mesh.extract(np.full((3, 4, 5), np.nan, _F), np.zeros((3, 4, 5), _F))          # unobserved: not looked at
    bad = [dict(D=np.ones((4, 5), _F)), dict(W=np.ones((3, 4, 4), _F)), dict(Fm=np.ones((3, 4, 5), _F)), dict(Fm=np.ones((2, 3, 4, 4), _F)),
           dict(voxel=(1, 0, 1)), dict(voxel=(1, 1)), dict(origin=(0, float("nan"), 0)), dict(min_weight=-1.0), dict(min_weight=float("nan")),
           dict(min_weight=float("inf")), dict(min_weight="x"), dict(Fm=np.ones((65, 3, 4, 5), _F)),
           dict(D=np.where(np.arange(60).reshape(3, 4, 5) == 7, np.nan, 1).astype(_F))]
    for kw in bad:
        with pytest.raises(ValueError):
            mesh.extract(**dict(dict(D=D, W=W), **kw))
    with pytest.raises(ValueError):
        mesh.write_ply("unused.ply", dict(vertices=np.zeros((2, 3), _F), faces=np.zeros((0, 3), np.int32), normal=None), colour=np.zeros((3, 3), _F))


def test_the_fusion_settings_file_takes_tsdf_mesh(tmp_path):
    from be_hip import workflow as wf
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    vol = dict(tsdf_dims=(8, 4, 6), tsdf_origin=(-0.5, 0, 0.25), tsdf_voxel=(0.5, 0.25, 0.125))
    np.savez(tmp_path / "vol.npz", poses=poses, **vol)
    assert "tsdf_mesh" not in wf.load_fusion(str(tmp_path / "vol.npz"))
    np.savez(tmp_path / "mesh.npz", poses=poses, tsdf_mesh=1, **vol)
    cfg = wf.load_fusion(str(tmp_path / "mesh.npz"))
    assert cfg["tsdf_mesh"] == 1 and set(cfg["tsdf"]) == {"dims", "origin", "voxel", "trunc"}
    np.savez(tmp_path / "off.npz", poses=poses, tsdf_mesh=0)
    assert wf.load_fusion(str(tmp_path / "off.npz"))["tsdf_mesh"] == 0
    np.savez(tmp_path / "lone.npz", poses=poses, tsdf_mesh=1)
    with pytest.raises(ValueError, match="tsdf_dims.*tsdf_origin.*tsdf_voxel"):
        wf.load_fusion(str(tmp_path / "lone.npz"))
    for bad in (-1, 1.5):
        np.savez(tmp_path / "bad.npz", poses=poses, tsdf_mesh=bad, **vol)
        with pytest.raises(ValueError):
            wf.load_fusion(str(tmp_path / "bad.npz"))
