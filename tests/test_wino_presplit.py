"""The pre-split Winograd weights (be_wino.hip: k_wino_pack_split) and the split-bf16 GEMM that reads them (k_wino_gemm_ps).

CPU: the packed size (fp32 U, then three bf16 planes of U with cout padded to 128).  GPU: the planes are a round-to-nearest-even split
of the packed fp32 U in the GEMM's block layout; the GEMM gives the bits of the round-7 kernel that split both operands in the loop,
for the six LocalStage layer shapes at every batch regime, padded channel counts and non-finite inputs.  That kernel left the library
when k_wino_gemm_ps had replaced it; its bits are tests/golden/wino_presplit_bits.json, the sha256 digests of _outputs() recorded with
the library of commit d45619f (the last one that held it) under its knob BE_WINO_BF6_R7=1, read once per process:

    BE_WINO_BF6_R7=1 BE_LIB_DIR=<directory with that commit's libblurry_edges_hip.so> python tests/test_wino_presplit.py --record

(that commit's default arm gave the same digests in the same recording run).  Without BE_LIB_DIR it records the library in the tree:
do that only for a change that is meant to move bits, and say so.  The inputs are seeded on the CPU."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from test_wino_split_bf16 import LAYERS, split3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wino_presplit_bits.json")
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
    """-> {case: sha256 of the Winograd layer's output} on fixed inputs under this process's GEMMs"""
    from be_hip import native
    out = {}

    def run(name, x, cin, cout, seed):
        w, b = _weights(cin, cout, seed)
        uw, ub = native.wino_pack(w.to(DEV), b.to(DEV))
        y, _ = native.wino_conv3x3(x, uw, ub, cout, act=1)
        out[name] = hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()

    for i, (cin, cout) in enumerate(LAYERS + ODD):
        g = torch.Generator().manual_seed(1000 + i)
        x4 = torch.randn(max(BATCHES), 6, 6, cin, generator=g).to(DEV)
        for n in BATCHES:
            run(f"l{i}_n{n}", x4[:n].contiguous(), cin, cout, 200 + i)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(64, 6, 6, 256, generator=g)
    x[3, 2, 2, 5] = float("inf")
    x[9, 0, 4, 17] = float("-inf")
    x[20, 5, 5, 100] = float("nan")
    run("nonfinite", x.to(DEV), 256, 256, 7)
    return out


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
    """Default GEMM (B from the planes) against the recorded bits of the round-7 kernel (both operands split in the loop): the six
    layer shapes and two padded ones at 3 / 700 / 1501 / 4096 patches, and a batch with inf / NaN inputs - bit for bit."""
    assert os.environ.get("BE_WINO_F32") in (None, "", "0"), \
        "BE_WINO_F32 is set in this environment: the fp32 GEMMs would run, not the split-bf16 GEMM whose bits are pinned here"
    with open(GOLDEN) as f:
        old = json.load(f)["digests"]
    new = _outputs()
    assert sorted(old) == sorted(new)
    bad = [k for k in new if new[k] != old[k]]
    assert not bad, bad


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: [BE_LIB_DIR=<directory of the library to record>] python tests/test_wino_presplit.py --record")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "blurry-edges_amd"), os.path.join(ROOT, "tests")]
    from be_hip import native as n
    n.lib()
    digests = _outputs()
    with open(os.path.join(os.path.dirname(n.LIB_PATH), "BUILD_INFO.json")) as f:       # written by build() next to the library
        built = json.load(f)
    with open(GOLDEN, "w") as f:
        json.dump({"library_git_head": built.get("git_head"), "library_dirty": built.get("dirty"), "digests": digests}, f, indent=1)
        f.write("\n")
    print(f"recorded {len(digests)} digests of {n.LIB_PATH} in {GOLDEN}")
