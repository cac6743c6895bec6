"""The asymmetric LDS ring of layer0's split-bf16 loop (be_conv_pm_bf6.hip: k_conv_pm_bf6): three A slots and two B slots of the 9
real pieces, B(c + 2) then A(c + 3) fetched at the top of chunk c, three workgroups per CU - against the recorded bits of the ring of
four whole stages that it replaced.  That ring left the library; its bits are tests/golden/l0_ring_bits.json, the "y" digests of
run_cases(False) recorded with the library of commit d45619f (the last one that held it) under its knob BE_BF6_RING4=1, read once per
process:

    BE_BF6_RING4=1 BE_LIB_DIR=<directory with that commit's libblurry_edges_hip.so> python tests/test_bf6_ring3.py --record

(without BE_LIB_DIR it records the library in the tree: do that only for a change that is meant to move bits, and say so).  Every
operand comes from numpy's default_rng or be_hip.synth on the CPU.

What such a ring can get wrong, at the smallest shapes that reach it: a slot overwritten before its fragments were read or read before
its DMA landed, A and B of different chunks paired, a B piece dealt to no wave or to the wrong place in the 9-KB slot, a padding piece
fetched over a neighbour.  The slot patterns of a 3-ring and a 2-ring repeat every 6 chunks; the walks here are 16 (corner pixel,
64 channels: 2 x 4 taps x 2 halves), 24, 28, 36, 40 and 58 (interior pixel, 96 channels + the 1x1 over 64) chunks long, with 4, 6 and
9 taps and the seam into the 1x1 segment.

Exact-product operands (test_split_bf16_interleave.py): every partial sum is an fp32 value, so a stale or swapped slot shows as a wrong
bit, not inside a tolerance; and a random-normal set with bias and Smish.  Rows 96-127 of every weight plane - padding that no fragment
read touches and the new ring does not fetch - are NaN in a second copy of the planes: the output must not move."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from test_layer0_split_bf16 import COUT, _pack
from test_split_bf16_interleave import _exact_f32, _l0_ref, _sparse_rows, _three_piece

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "l0_ring_bits.json")
DEV = "cuda:0"
CONFIGS = [(64, 0), (96, 64)]                          # layer0's two launches: 64 -> 96, and 96 -> 96 with the fused 1x1 over 64
MAPS = [(3, 3), (11, 11)]                              # every pixel but one on the border; the real map
NS = (1, 3, 130)                                       # one image, a few, a full 128-image group and two rows of a second
SETS = ("exact_a", "exact_b", "normal")
CASES = [(cin, cin2, h, w, kind) for cin, cin2 in CONFIGS for h, w in MAPS for kind in SETS]
STAGE_NS = (16, 130)


def _key(cin, cin2, h, w, kind, n):
    return f"c{cin}_x{cin2}_{h}x{w}_{kind}_n{n}"


def _operands(cin, cin2, h, w, kind):
    """-> x, x2, wt, w2, bias (float64 numpy, each an fp32 value), act"""
    n, ktot = max(NS), 9 * cin + cin2
    rng = np.random.default_rng(2500 + cin + cin2 + 7 * h + SETS.index(kind))
    if kind == "exact_a":                              # x carries all three pieces; at most 16 non-zero weights per output channel
        x = _three_piece((n, h, w, cin), rng)
        x2 = _three_piece((n, h, w, cin2), rng) if cin2 else None
        wall = _sparse_rows(COUT, ktot, 16, rng)
    elif kind == "exact_b":                            # the weights carry the pieces; a window sees at most 10 + 6 non-zeros of an image
        x = _sparse_rows(n, h * w * cin, 10, rng).reshape(n, h, w, cin)
        x2 = _sparse_rows(n, h * w * cin2, 6, rng).reshape(n, h, w, cin2) if cin2 else None
        wall = _three_piece((COUT, ktot), rng)
    else:
        f = lambda *s: rng.standard_normal(s).astype(np.float32).astype(np.float64)
        x, x2 = f(n, h, w, cin), (f(n, h, w, cin2) if cin2 else None)
        wall = (f(COUT, ktot) * np.sqrt(2.0 / ktot)).astype(np.float32).astype(np.float64)
    wt = wall[:, :9 * cin].reshape(COUT, cin, 3, 3).copy()
    w2 = wall[:, 9 * cin:].reshape(COUT, cin2, 1, 1).copy() if cin2 else None
    bias = np.zeros(COUT) if kind != "normal" else (0.1 * rng.standard_normal(COUT)).astype(np.float32).astype(np.float64)
    return x, x2, wt, w2, bias, (1 if kind == "normal" else 0)


def _poisoned(planes):
    """a copy of the planes with rows 96-127 of every [chunk][plane][128 rows][16 bf16] block set to NaN"""
    p = planes.clone()
    p.view(torch.int16).view(-1, 3, 128, 16)[:, :, 96:, :] = 0x7FC0
    assert torch.isnan(p.view(torch.bfloat16).view(-1, 3, 128, 16)[:, :, 96:, :]).all()
    return p


def _digest(y):
    return hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest()


def _stage_logits():
    import models
    from be_hip import synth
    m = models.LocalStage()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.local_stage_state_dict().items()})
    m = m.to(DEV).eval()
    assert m.winograd is True
    x = torch.from_numpy(np.asarray(synth.uniform_patches(max(STAGE_NS), name="bf6_ring3"), dtype=np.float32)).to(DEV)
    with torch.no_grad():
        return {n: m(x[:n].contiguous()).cpu().numpy().copy() for n in STAGE_NS}


def run_cases(check_exact):
    """This process's arm: per case the digest of the output, of the output on the poisoned planes and - exact sets, check_exact -
    the number of elements that differ from the float64 convolution; and LocalStage's logits."""
    from be_hip import native
    f32 = lambda a: None if a is None else torch.from_numpy(a.astype(np.float32))
    out = {}
    for cin, cin2, h, w, kind in CASES:
        x, x2, wt, w2, bias, act = _operands(cin, cin2, h, w, kind)
        _, pb, planes, _ = _pack(native, f32(wt), f32(bias), f32(w2))
        bad = _poisoned(planes)
        ref = _exact_f32(_l0_ref(x, wt, x2, w2)) if check_exact and kind != "normal" else None
        xd, x2d = f32(x).to(DEV), (f32(x2).to(DEV) if cin2 else None)
        for n in NS:
            xn, x2n = xd[:n].contiguous(), (x2d[:n].contiguous() if cin2 else None)
            y = native.conv3x3_pm_bf6(xn, planes, pb, COUT, act=act, x2=x2n).cpu().numpy()
            yp = native.conv3x3_pm_bf6(xn, bad, pb, COUT, act=act, x2=x2n).cpu().numpy()
            rec = {"y": _digest(y), "y_poisoned_planes": _digest(yp), "finite": bool(np.isfinite(y).all())}
            if ref is not None:
                rec["wrong"] = int((y != ref[:n]).sum())
            out[_key(cin, cin2, h, w, kind, n)] = rec
    for n, v in _stage_logits().items():
        out[f"stage_n{n}"] = {"y": _digest(v), "finite": bool(np.isfinite(v).all())}
    return out


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


@pytest.fixture(scope="module")
def this_arm(native):
    return run_cases(True)


@pytest.fixture(scope="module")
def golden():
    """{case: digest of y} of the same cases on the ring of four whole stages"""
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cin2,h,w,kind", CASES, ids=[_key(*c, 0)[:-3] for c in CASES])
def test_layer0_bits_on_either_ring_with_nan_in_the_padding_rows(this_arm, golden, cin, cin2, h, w, kind):
    for n in NS:
        k = _key(cin, cin2, h, w, kind, n)
        a = this_arm[k]
        assert a["finite"], k
        if kind != "normal":
            assert a["wrong"] == 0, (k, a["wrong"])                  # the float64 convolution, bit for bit
        assert a["y_poisoned_planes"] == a["y"], k                   # rows 96-127 of the planes reach no output
        assert a["y"] == golden[k], k                                # the two rings: the same bits


@pytest.mark.gpu
def test_local_stage_logits_are_bit_equal_on_either_ring(this_arm, golden):
    for n in STAGE_NS:
        a = this_arm[f"stage_n{n}"]
        assert a["finite"]
        assert a["y"] == golden[f"stage_n{n}"], n


def _normal_on_device(native, cin, cin2, h, w):
    x, x2, wt, w2, bias, act = _operands(cin, cin2, h, w, "normal")
    f32 = lambda a: torch.from_numpy(a.astype(np.float32))
    _, pb, planes, _ = _pack(native, f32(wt), f32(bias), f32(w2))
    return f32(x), f32(x2), planes, pb, act


@pytest.mark.gpu
def test_ten_runs_are_bit_identical(native):
    """A slot read before its DMA has landed, or overwritten while a slower wave still reads it, shows here."""
    x, x2, planes, pb, act = _normal_on_device(native, 96, 64, 11, 11)
    xd, x2d = x.to(DEV), x2.to(DEV)
    first = native.conv3x3_pm_bf6(xd, planes, pb, COUT, act=act, x2=x2d)
    assert torch.isfinite(first).all()
    for _ in range(9):
        assert torch.equal(native.conv3x3_pm_bf6(xd, planes, pb, COUT, act=act, x2=x2d), first)


@pytest.mark.gpu
def test_nonfinite_values_of_one_image_stay_in_that_image(native):
    """An image is a row of the tile: NaN and +-inf in it (x and x2, first and last chunk of the walk) reach its outputs and no other's."""
    x, x2, planes, pb, act = _normal_on_device(native, 96, 64, 11, 11)
    clean = native.conv3x3_pm_bf6(x.to(DEV), planes, pb, COUT, act=act, x2=x2.to(DEV)).cpu().numpy()
    assert np.isfinite(clean).all()
    x, x2 = x.clone(), x2.clone()
    x[5, :, :, 0] = float("nan")                       # channel 0: the first chunk of every tap
    x2[77, :, :, 63] = float("inf")                    # the last chunk of the walk
    x[129, :, :, 95] = float("-inf")                   # second group, which holds two images
    y = native.conv3x3_pm_bf6(x.to(DEV), planes, pb, COUT, act=act, x2=x2.to(DEV)).cpu().numpy()
    rows = [5, 77, 129]
    assert not np.isfinite(y[rows]).any()
    keep = np.setdiff1d(np.arange(max(NS)), rows)
    assert np.array_equal(y[keep], clean[keep])


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: [BE_LIB_DIR=<directory of the library to record>] python tests/test_bf6_ring3.py --record")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "blurry-edges_amd"), os.path.join(ROOT, "tests")]
    from be_hip import native as n
    n.lib()
    cases = run_cases(False)
    assert all(v["finite"] for v in cases.values())
    with open(os.path.join(os.path.dirname(n.LIB_PATH), "BUILD_INFO.json")) as f:       # written by build() next to the library
        built = json.load(f)
    with open(GOLDEN, "w") as f:
        json.dump({"library_git_head": built.get("git_head"), "library_dirty": built.get("dirty"),
                   "digests": {k: v["y"] for k, v in cases.items()}}, f, indent=1)
        f.write("\n")
    print(f"recorded {len(cases)} digests of {n.LIB_PATH} in {GOLDEN}")
