"""The pre-split Winograd weights (be_wino.hip: k_wino_pack_split) and the split-bf16 GEMM that reads them (k_wino_gemm_ps).

CPU: the packed size (fp32 U, then three bf16 planes of U with cout padded to 128).  GPU: the planes are a round-to-nearest-even split
of the packed fp32 U in the GEMM's block layout; the GEMM gives the bits of the round-7 kernel that splits both operands in the loop
(BE_WINO_BF6_R7=1, in a child process: the knob is read once per process) for the six LocalStage layer shapes at every batch regime,
padded channel counts and non-finite inputs."""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from test_wino_split_bf16 import LAYERS, split3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BATCHES = (3, 700, 1501, 4096)          # plane-major, plane-major, tile-major with a partial row tile, tile-major full tiles
ODD = [(64, 100), (32, 164)]             # cout_pad32 = 128 / 192: N tiles past cout_pad (zero rows of the planes)


def _lib():
    from be_hip import native
    return native.lib()


def _positions(lib):
    return 5 * (lib.be_wino_tile_rows() + 2)


def test_packed_size_is_u_then_three_bf16_planes():
    lib = _lib()
    npos = _positions(lib)
    for cin, cout in LAYERS + ODD + [(32, 4), (384, 384)]:
        cp32, cp128 = (cout + 31) // 32 * 32, (cout + 127) // 128 * 128
        got = lib.be_wino_packed_floats(cout, cin)
        assert got == npos * cp32 * cin + npos * cp128 * cin * 3 // 2, (cout, cin)
        assert (npos * cp32 * cin) % 4 == 0                          # the planes start 16-byte aligned
    assert lib.be_wino_packed_floats(64, 48) == 0


# ---------------------------------------------------------------------------------------------------------------------- GPU

def _weights(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) * np.sqrt(2.0 / (9 * cin))
    b = 0.1 * torch.randn(cout, generator=g)
    return w, b


def _outputs():
    """Digests of the Winograd layer outputs on fixed inputs under this process's GEMMs (plus one small array for diagnostics)."""
    from be_hip import native
    out = {}

    def run(name, x, cin, cout, seed):
        w, b = _weights(cin, cout, seed)
        uw, ub = native.wino_pack(w.to(DEV), b.to(DEV))
        y, _ = native.wino_conv3x3(x, uw, ub, cout, act=1)
        y = y.cpu().numpy()
        out[name] = np.frombuffer(hashlib.sha256(y.tobytes()).digest(), dtype=np.uint8)
        out[name + "_head"] = y.reshape(-1)[:4096].copy()

    for i, (cin, cout) in enumerate(LAYERS + ODD):
        g = torch.Generator(device=DEV).manual_seed(1000 + i)
        x4 = torch.randn(max(BATCHES), 6, 6, cin, device=DEV, generator=g)
        for n in BATCHES:
            run(f"l{i}_n{n}", x4[:n].contiguous(), cin, cout, 200 + i)
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(64, 6, 6, 256, device=DEV, generator=g)
    x[3, 2, 2, 5] = float("inf")
    x[9, 0, 4, 17] = float("-inf")
    x[20, 5, 5, 100] = float("nan")
    run("nonfinite", x, 256, 256, 7)
    return out


_CHILD = r'''
import os, sys
import numpy as np
sys.path[:0] = [os.environ["BE_ROOT"], os.path.join(os.environ["BE_ROOT"], "blurry-edges_amd"), os.path.join(os.environ["BE_ROOT"], "tests")]
import test_wino_presplit as t
np.savez(os.environ["BE_OUT"], **t._outputs())
'''


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


@pytest.mark.gpu
def test_planes_are_the_rne_split_of_u_in_block_layout(native):
    lib = native.lib()
    npos = _positions(lib)
    for i, (cin, cout) in enumerate([LAYERS[0], LAYERS[2]] + ODD):
        w, b = _weights(cin, cout, 300 + i)
        uw, _ = native.wino_pack(w.to(DEV), b.to(DEV))
        pw = uw.cpu().numpy()
        cp32, nt, kc = (cout + 31) // 32 * 32, (cout + 127) // 128, cin // 16
        nu = npos * cp32 * cin
        assert pw.size == lib.be_wino_packed_floats(cout, cin)
        u = np.zeros((npos, nt * 128, cin), np.float32)
        u[:, :cp32] = pw[:nu].reshape(npos, cp32, cin)
        assert np.all(u[:, cout:cp32] == 0) and np.isfinite(u).all()
        # expected: [position][N tile][K chunk][plane][row][half][8] with the halves of rows 8-15, 24-31, ... swapped
        pieces = np.stack([p.view(np.uint32) >> 16 for p in split3(u)]).astype(np.uint16)        # [3][npos][rows][cin]
        e = pieces.reshape(3, npos, nt, 128, kc, 2, 8).transpose(1, 2, 4, 0, 3, 5, 6).copy()
        swap = ((np.arange(128) >> 3) & 1).astype(bool)
        e[:, :, :, :, swap] = e[:, :, :, :, swap][..., ::-1, :]
        got = pw[nu:].view(np.uint16).reshape(npos, nt, kc, 3, 128, 2, 8)
        assert np.array_equal(got, e), (cin, cout)


@pytest.mark.gpu
def test_presplit_gemm_gives_the_round7_kernels_bits(native):
    """Default GEMM (B from the planes) against BE_WINO_BF6_R7=1 (both operands split in the loop) in a fresh child process: the six
    layer shapes and two padded ones at 3 / 700 / 1501 / 4096 patches, and a batch with inf / NaN inputs - bit for bit.  Both arms run
    in child processes whose knobs are set here, whatever the suite's environment holds."""
    def arm(d, name, **knobs):
        env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, name + ".npz"))
        for k in ("BE_WINO_F32", "BE_WINO_BF6_R7"):
            env.pop(k, None)
        env.update(knobs)
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return dict(np.load(os.path.join(d, name + ".npz")))

    with tempfile.TemporaryDirectory() as d:
        new = arm(d, "default")
        old = arm(d, "r7", BE_WINO_BF6_R7="1")
    assert sorted(old) == sorted(new)
    bad = [k for k in new if new[k].tobytes() != old[k].tobytes()]
    assert not bad, bad
