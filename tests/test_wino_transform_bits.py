"""The Winograd transform kernels (be_wino.hip: k_wino_in, k_wino_out, k_wino_out_in, k_wino_out_res_in<STORE_Y>, k_wino_out_pool2,
k_pool_wino_in<STORE_P>) pinned to recorded bits.

The other Winograd tests compare the library with itself (chained against unchained, folded against float64 at 1e-5): a change
mirrored in every kernel - `o + res + bias` for `o + bias + res`, say - passes them.  Here every case's output bytes are hashed
(sha256) and compared with tests/golden/wino_transform_bits.json, which was recorded with the library of the commit BEFORE the six
kernels were rebuilt from one tile loop per side:

    BE_LIB_DIR=<directory with that commit's libblurry_edges_hip.so> python tests/test_wino_transform_bits.py --record

(without BE_LIB_DIR it records the library in the tree: do that only for a change that is meant to move bits, and say so).  The
digests are stable on the MI355X: the inputs are seeded on the CPU, and the GEMMs' bits depend on neither batch, group count nor
stream (test_wino_ds_fold.py).

Cases, at n = 3 (plane-major, a partial GEMM tile) and n = 1024 (where a layer whose outputs pad to a multiple of 128 turns
tile-major), for (cin, cmid, cout) = (32, 128, 96) - at 1024 a tile-major M feeds a plane-major V' - and (64, 128, 128), tile-major
throughout:
  conv        wino_conv3x3, residual none / tensor x act 0, 1, 2                          k_wino_in, k_wino_out
  pair        wino_conv3x3_pair                                                           k_wino_out_in, k_wino_out
  chain       two chained blocks without / with a residual / with test_wino_chain's special-value residual: y of block one and
              the output of block two                                                     k_wino_out_res_in<1>
  ds          three folded blocks, the middle one with x_in_v, next_cmid and store_y=False  k_wino_out_res_in<0>
              (the fold wants conv1's and conv2's layouts equal, so (32, 128, 96) has no n = 1024 case: the library refuses it)
  pool        maxpool_wino_in on test_wino_chain._pool_input(n, 32) and a chained block   k_pool_wino_in<1>
and LocalStage's logits on synth weights and patches at n = 1, 65, 1100: in this process (the default arm: k_pool_wino_in<0>,
k_wino_out_res_in<0>, k_wino_out_pool2 without a residual) and in ONE child with BE_WINO_DS_GEMM=1 (read once per process:
k_wino_out_pool2 and the chained k_wino_out_res_in<1> with a residual tensor)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wino_transform_bits.json")
DEV = "cuda:0"
pytestmark = pytest.mark.gpu

BATCHES = (3, 1024)
SHAPES = ((32, 128, 96), (64, 128, 128))


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t).tobytes())
    return h.hexdigest()


def kernel_cases(native):
    """-> {case name: digest} of everything but the LocalStage logits, in a fixed order"""
    import test_wino_chain as twc
    import test_wino_ds_fold as tdf
    lib = native.lib()
    out = {}
    for shape in SHAPES:
        cin, c1, c2 = shape
        (u1, b1), (u2, b2), _, _ = twc.packs(native, shape)
        for n in BATCHES:
            tag = f"{cin}-{c1}-{c2} n={n}"
            g = torch.Generator().manual_seed(17 * n + c1)
            x = torch.randn(n, 6, 6, cin, generator=g).to(DEV)
            r = torch.randn(n, 6, 6, c1, generator=g).to(DEV)
            for res in (None, r):
                for act in (0, 1, 2):
                    y, _ = native.wino_conv3x3(x, u1, b1, c1, act=act, residual=res)
                    out[f"conv {tag} res={res is not None} act={act}"] = sha(y)
            y, _ = native.wino_conv3x3_pair(x, u1, b1, c1, u2, b2, c1, act1=1, act2=1, residual=r)
            out[f"pair {tag}"] = sha(y)
            for name, res in (("none", None), ("tensor", r)):
                out[f"chain {tag} res={name}"] = sha(*twc.two_blocks(native, shape, x, res, 1, 1, chained=True))
    for n in BATCHES:                                                   # test_wino_chain's special values through the residual
        g = torch.Generator().manual_seed(91 + n)
        x = torch.randn(n, 6, 6, 32, generator=g).to(DEV)
        r = torch.randn(n, 6, 6, 128, generator=g)
        r[0, :, :, :4] = 0.0
        r[0, 0, 0, 0], r[0, 0, 1, 1], r[0, 2, 3, 2], r[0, 5, 5, 3] = float("inf"), float("-inf"), float("nan"), -1000.0
        r[0, 3, 3, 0], r[0, 4, 1, 1] = -0.0, -1.0e30
        r[0, 1, 4, 77], r[0, 4, 4, 100] = float("inf"), float("nan")
        for act in (0, 1):
            y1, y2 = twc.two_blocks(native, (32, 128, 96), x, r.to(DEV), 1, act, chained=True)
            assert bool(torch.isnan(y1[0]).any()) and bool(torch.isfinite(y1[1:]).all())
            out[f"chain 32-128-96 n={n} res=special act={act}"] = sha(y1, y2)
    for cin, cm, c in SHAPES:
        p = tdf._block(native, cin, cm, c)
        nxt = lambda **kw: native.wino_conv3x3_pair_ds(None, *p["d1"], c, p["d2"][0], p["d2b"], p["dds"][0], c, x_in_v=True, cin=c, **kw)
        for n in BATCHES:
            if n >= 1024 and (cm % 128 == 0) != (c % 128 == 0):
                continue                                                # conv1's and conv2's layouts differ: no folded form
            x = torch.randn(n, 6, 6, cin, generator=torch.Generator().manual_seed(1430 + n + c)).to(DEV)
            need = max(lib.be_wino_pair_ds_workspace_floats(n, cin, cm, c), lib.be_wino_pair_ds_workspace_floats(n, c, c, c))
            ws = torch.full((need,), float("nan"), dtype=torch.float32, device=DEV)
            y1, _ = tdf._folded(native, p, x, cm, c, workspace=ws, next_cmid=c)
            none, _ = nxt(n=n, workspace=ws, next_cmid=c, store_y=False)
            z, _ = nxt(n=n, workspace=ws)
            assert none is None and bool(torch.isfinite(z).all())
            out[f"ds {cin}-{cm}-{c} n={n}"] = sha(y1, z)
    cmid = 128
    g = torch.Generator().manual_seed(7 + 32)
    (u1, b1), (u2, b2) = twc._conv(g, cmid, 32, native), twc._conv(g, cmid, cmid, native)
    for n in BATCHES:
        x = twc._pool_input(n, 32)
        ws = torch.full((lib.be_wino_pair_workspace_floats(n, 32, cmid, cmid),), float("nan"), dtype=torch.float32, device=DEV)
        pooled = native.maxpool_wino_in(x, cmid, ws)
        y = native.wino_conv3x3_pair_chain(torch.zeros_like(pooled), u1, b1, cmid, u2, b2, cmid, ws, x_in_v=True)
        out[f"pool c=32 n={n}"] = sha(pooled, y)
    return out


def logits_cases(arm, got):
    import test_wino_chain as twc
    return {f"logits {arm} n={n}": sha(got[f"n{n}_r0"]) for n in twc.LS_BATCHES}


def ds_gemm_child():
    """LocalStage's logits of a fresh process with BE_WINO_DS_GEMM=1 (the blocks' downsamples as separate row GEMMs)"""
    import test_wino_chain as twc
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, "ds_gemm.npz"))
        for k in twc.KNOBS:
            env.pop(k, None)
        env["BE_WINO_DS_GEMM"] = "1"
        r = subprocess.run([sys.executable, "-c", twc._CHILD], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return dict(np.load(os.path.join(d, "ds_gemm.npz")))


def all_cases(native):
    import test_wino_chain as twc
    out = kernel_cases(native)
    out.update(logits_cases("default", twc._logits()))
    out.update(logits_cases("BE_WINO_DS_GEMM=1", ds_gemm_child()))
    return out


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["digests"]


def first_difference(got, golden, prefix=None):
    want = {k: v for k, v in golden.items() if prefix is None or k.startswith(prefix)}
    assert list(got) == list(want), ("the cases are not the recorded ones", sorted(set(got) ^ set(want)))
    for k, v in got.items():
        print(k, v[:16], "ok" if v == want[k] else f"DIFFERS from {want[k][:16]}")
    return next((k for k, v in got.items() if v != want[k]), None)


def test_transform_kernels_give_the_recorded_bits(native, golden):
    got = kernel_cases(native)
    assert first_difference(got, {k: v for k, v in golden.items() if not k.startswith("logits ")}) is None


def test_local_stage_logits_give_the_recorded_bits(native, golden):
    import test_wino_chain as twc
    assert first_difference(logits_cases("default", twc._logits()), golden, "logits default ") is None


def test_local_stage_logits_with_separate_downsamples_give_the_recorded_bits(native, golden):
    assert first_difference(logits_cases("BE_WINO_DS_GEMM=1", ds_gemm_child()), golden, "logits BE_WINO_DS_GEMM=1 ") is None


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: [BE_LIB_DIR=<directory of the library to record>] python tests/test_wino_transform_bits.py --record")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "blurry-edges_amd"), os.path.join(ROOT, "tests")]
    from be_hip import native as n
    n.lib()
    digests = all_cases(n)
    info = os.path.join(os.path.dirname(n.LIB_PATH), "BUILD_INFO.json")              # written by build() next to the library
    with open(info) as f:
        built = json.load(f)
    with open(GOLDEN, "w") as f:
        json.dump({"library_git_head": built.get("git_head"), "library_dirty": built.get("dirty"), "digests": digests}, f, indent=1)
        f.write("\n")
    print(f"recorded {len(digests)} digests of {n.LIB_PATH} in {GOLDEN}")
