"""The wave grid of the split-bf16 GEMM k_wino_gemm_ps (be_wino.hip): the workgroup's four waves stacked in M (4x1: wave w owns rows
32 w .. 32 w + 31 and all 128 columns, one A fragment split per chunk) against the 2x2 grid of rounds 8-15 (BE_WINO_WAVES22=1), in
which two waves split the same 64 A rows.  The grid changes which wave computes an element, never how: both arms must give the same
bits everywhere.

What a wave grid can get wrong, at the smallest shapes that reach it: a wave's row or column offset in the fragment reads or in the
stores (2, 66 and 130 rows: wave 0 alone, wave 2 with two real rows and wave 3 with none, a second M tile of two rows), a column
block's mask (cout = 100: block 3 partly masked; 256: two N tiles), a B fragment in the wrong accumulator or a stale register set
(exact-product operands - test_split_bf16_interleave.py - on 1, 3 and 6 chunks, with and without the second K segment of 1 and 2
chunks, both buffer layouts: any wrong, missing or repeated piece moves a bit of the float64 result), non-finite values leaving
their row, and run-to-run differences.  The knob is read once per process, so each arm runs in one child process which does every
case and returns SHA-256 digests of the outputs (equal digests = equal bits) and the list of cases that missed float64."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from test_split_bf16_interleave import _exact_f32, _packed, _sparse_rows, _three_piece
from test_wino_ds_fold import LIVE, NLIVE, NPOS, _block, _folded, _packed_from_u, _sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NS = (1, 33, 65)                                            # maps: 2, 66 and 130 rows per position
COUTS = (100, 256)
CINS = (16, 48, 96)                                         # 1 chunk, 3 (the loop ends behind body 0), 6
CIN_EXTS = (0, 16, 32)                                      # no second segment, 1 and 2 chunks more at the live positions
ROW_MS = (2, 66, 130)
PAIR_BLOCKS = [(32, 64, 100), (64, 96, 256)]                # cin -> cmid -> cout with the 1x1 downsample cin -> cout folded in
LS_BATCHES = (3, 130)
KNOB = "BE_WINO_WAVES22"


def _digest(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _lay(a, tm):
    """[positions][tiles][c] -> the buffer layout (tile-major: [tiles][positions][c])"""
    return np.ascontiguousarray(a.transpose(1, 0, 2)) if tm else np.ascontiguousarray(a)


def _gemm_exact(native, out, errors):
    nmax = max(NS)
    for cin in CINS:
        rng = np.random.default_rng(2100 + cin)
        v = _three_piece((NPOS, 2 * nmax, cin), rng)
        vx = {ce: _three_piece((NPOS, 2 * nmax, ce), rng) for ce in CIN_EXTS if ce}
        for cout in COUTS:
            u = _sparse((NPOS, cout, cin), 10, rng)
            pw = _packed_from_u(native, u, cout, cin)
            first = v @ u.transpose(0, 2, 1)
            for ce in CIN_EXTS:
                if ce:
                    uds = _sparse((NLIVE, cout, ce), 10, rng)
                    uds_all = np.zeros((NPOS, cout, ce))
                    uds_all[LIVE] = uds
                    pds = _packed_from_u(native, uds, cout, ce)
                    assert (np.abs(v) @ np.abs(u).transpose(0, 2, 1) + np.abs(vx[ce]) @ np.abs(uds_all).transpose(0, 2, 1)).max() < 128.0
                    ref = _exact_f32(first + vx[ce] @ uds_all.transpose(0, 2, 1))
                else:
                    assert (np.abs(v) @ np.abs(u).transpose(0, 2, 1)).max() < 128.0
                    ref = _exact_f32(first)
                for n in NS:
                    for tm in (False, True):
                        vd = torch.from_numpy(_lay(v[:, :2 * n], tm).astype(np.float32)).to(DEV)
                        if ce:
                            vxd = torch.from_numpy(_lay(vx[ce][:, :2 * n], tm).astype(np.float32)).to(DEV)
                            m = native.wino_gemms_ext(vd, pw, n, cin, cout, vxd, pds, ce, tile_major=tm)
                        else:
                            m = native.wino_gemms_ext(vd, pw, n, cin, cout, tile_major=tm)
                        key = f"gemm_cin{cin}_cout{cout}_ext{ce}_n{n}_tm{int(tm)}"
                        out[key] = _digest(m)
                        got = m.cpu().numpy()
                        bad = np.argwhere(got != _lay(ref[:, :2 * n], tm))
                        if bad.size:
                            errors.append(f"{key}: {len(bad)} elements differ from float64, first {bad[:4].tolist()}")


def _rows_exact(native, out, errors):
    for k in CINS:
        rng = np.random.default_rng(2200 + k)
        x = _three_piece((max(ROW_MS), k), rng)
        w = _sparse_rows(max(COUTS), k, 20, rng)
        xd = torch.from_numpy(x.astype(np.float32)).to(DEV)
        for n in COUTS:
            assert (np.abs(x) @ np.abs(w[:n]).T).max() < 128.0
            ref = _exact_f32(x @ w[:n].T)
            planes = native.gemm_rows_bf6_pack(_packed(w[:n]), n, k)
            for m in ROW_MS:
                y = native.gemm_rows_bf6(xd[:m].contiguous(), planes, n)
                key = f"rows_k{k}_n{n}_m{m}"
                out[key] = _digest(y)
                bad = np.argwhere(y.cpu().numpy() != ref[:m])
                if bad.size:
                    errors.append(f"{key}: {len(bad)} elements differ from float64, first {bad[:4].tolist()}")


def _pair_ds(native, out, errors):
    for cin, cm, c in PAIR_BLOCKS:
        p = _block(native, cin, cm, c)
        x = torch.randn(max(NS), 6, 6, cin, generator=torch.Generator().manual_seed(2300 + c)).to(DEV)
        for n in NS:
            y = _folded(native, p, x[:n].contiguous(), cm, c)[0]
            key = f"pair_ds_{cin}_{cm}_{c}_n{n}"
            out[key] = _digest(y)
            if not bool(torch.isfinite(y).all()):
                errors.append(f"{key}: non-finite output")


def _rand_gemm(native, cin, cout, ce, n, seed):
    """random operands of the GEMMs given directly in the transform domain: (v, packed u, vx, packed u_ds)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(NPOS, 2 * n, cin, generator=g)
    u = (torch.randn(NPOS, cout, cin, generator=g) * float(np.sqrt(1.0 / cin))).numpy()
    vx = torch.randn(NPOS, 2 * n, ce, generator=g)
    uds = (torch.randn(NLIVE, cout, ce, generator=g) * float(np.sqrt(1.0 / ce))).numpy()
    return v, _packed_from_u(native, u, cout, cin), vx, _packed_from_u(native, uds, cout, ce)


def _nonfinite(native, out, errors):
    """NaN, +inf and -inf in channels 16-31 (chunk 1: an odd chunk, multiplied out of the second register set) of ONE A row - tile row
    40 of 66 (wave 1 of the 4x1 grid, wave 0's second fragment of the 2x2 grid) at one live position - of V, and of Vx"""
    cin, cout, ce, n, z, t = 48, 100, 32, 33, LIVE[3], 40
    v, pw, vx, pds = _rand_gemm(native, cin, cout, ce, n, 2400)
    run = lambda a, b: native.wino_gemms_ext(a.to(DEV), pw, n, cin, cout, None if b is None else b.to(DEV), None if b is None else pds, ce if b is not None else 0)
    poison = lambda a: [a.__setitem__((z, t, ch), val) for ch, val in ((17, float("nan")), (20, float("inf")), (25, float("-inf")))]
    vp, vxp = v.clone(), vx.clone()
    poison(vp)
    poison(vxp)
    for name, clean, dirty in (("plain", run(v, None), run(vp, None)), ("ext_v", run(v, vx), run(vp, vx)), ("ext_vx", run(v, vx), run(v, vxp))):
        key = f"nonfinite_{name}"
        out[key] = _digest(dirty)
        if not bool(torch.isfinite(clean).all()):
            errors.append(f"{key}: the clean run is not finite")
        if bool(torch.isfinite(dirty[z, t]).any()):
            errors.append(f"{key}: finite values in the poisoned row")
        c2, d2 = clean.clone(), dirty.clone()
        c2[z, t] = 0.0
        d2[z, t] = 0.0
        if not torch.equal(c2.view(torch.int32), d2.view(torch.int32)):
            errors.append(f"{key}: another row than the poisoned one differs from the clean run")
    # the row GEMM: row 40 of 66
    g = torch.Generator().manual_seed(2401)
    x, w = torch.randn(66, 48, generator=g), torch.randn(100, 48, generator=g) * float(np.sqrt(1.0 / 48))
    planes = native.gemm_rows_bf6_pack(_packed(w.numpy()), 100, 48)
    clean = native.gemm_rows_bf6(x.to(DEV), planes, 100)
    for ch, val in ((17, float("nan")), (20, float("inf")), (25, float("-inf"))):
        x[40, ch] = val
    dirty = native.gemm_rows_bf6(x.to(DEV), planes, 100)
    out["nonfinite_rows"] = _digest(dirty)
    keep = [r for r in range(66) if r != 40]
    if bool(torch.isfinite(dirty[40]).any()) or not torch.equal(clean[keep].view(torch.int32), dirty[keep].view(torch.int32)):
        errors.append("nonfinite_rows: the poisoned row is finite or another row moved")


def _ten_runs(native, out, errors):
    cin, cout, ce, n = 96, 256, 32, 65
    v, pw, vx, pds = _rand_gemm(native, cin, cout, ce, n, 2500)
    vd, vxd = v.to(DEV), vx.to(DEV)
    for name, run in (("plain", lambda: native.wino_gemms_ext(vd, pw, n, cin, cout)),
                      ("ext", lambda: native.wino_gemms_ext(vd, pw, n, cin, cout, vxd, pds, ce))):
        runs = {_digest(run()) for _ in range(10)}
        out[f"ten_runs_{name}"] = sorted(runs)[0]
        if len(runs) != 1:
            errors.append(f"ten_runs_{name}: {len(runs)} different results in ten runs")
    p = _block(native, 64, 96, 256)
    x = torch.randn(65, 6, 6, 64, generator=torch.Generator().manual_seed(2501)).to(DEV)
    ws, runs = None, set()
    for _ in range(10):
        y, ws = _folded(native, p, x, 96, 256, workspace=ws)
        runs.add(_digest(y))
    out["ten_runs_pair_ds"] = sorted(runs)[0]
    if len(runs) != 1:
        errors.append(f"ten_runs_pair_ds: {len(runs)} different results in ten runs")


def _logits(native, out, errors):
    import models
    from be_hip import synth
    m = models.LocalStage()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.local_stage_state_dict().items()})
    m = m.to(DEV).eval()
    assert m.winograd is True
    x = torch.from_numpy(np.asarray(synth.uniform_patches(max(LS_BATCHES), name="wino_wave_grid"), dtype=np.float32)).to(DEV)
    with torch.no_grad():
        for n in LS_BATCHES:
            y = m(x[:n].contiguous())
            out[f"logits_n{n}"] = _digest(y)
            if not bool(torch.isfinite(y).all()):
                errors.append(f"logits_n{n}: non-finite logits")


def run_cases():
    """every case in this process's arm -> {"digests": {case: sha256 of the output}, "errors": [what missed its own check]}"""
    from be_hip import native
    native.lib()
    out, errors = {}, []
    for part in (_gemm_exact, _rows_exact, _pair_ds, _nonfinite, _ten_runs, _logits):
        part(native, out, errors)
    torch.cuda.synchronize()
    return {"digests": out, "errors": errors}


_CHILD = r'''
import json, os, sys
sys.path[:0] = [os.environ["BE_ROOT"], os.path.join(os.environ["BE_ROOT"], "blurry-edges_amd"), os.path.join(os.environ["BE_ROOT"], "tests")]
import test_wino_wave_grid as t
with open(os.environ["BE_OUT"], "w") as f:
    json.dump(t.run_cases(), f)
'''


def _child(d, name, **knobs):
    env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, name + ".json"))
    env.pop(KNOB, None)
    env.update(knobs)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-4000:])
    with open(os.path.join(d, name + ".json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def arms():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    with tempfile.TemporaryDirectory() as d:                    # one after the other
        return {"4x1": _child(d, "default"), "2x2": _child(d, "waves22", **{KNOB: "1"})}


def _cases(arms, prefix):
    keys = sorted(k for k in arms["4x1"]["digests"] if k.startswith(prefix))
    assert keys and keys == sorted(k for k in arms["2x2"]["digests"] if k.startswith(prefix))
    return keys


def _no_errors(arms, prefix):
    for arm, got in arms.items():
        bad = [e for e in got["errors"] if e.startswith(prefix)]
        assert not bad, (arm, bad[:8])


def _arms_bit_equal(arms, prefix):
    diff = [k for k in _cases(arms, prefix) if arms["4x1"]["digests"][k] != arms["2x2"]["digests"][k]]
    assert not diff, diff[:8]


def test_exact_products_equal_float64_on_both_grids(arms):
    """every n x cout x cin x cin_ext x layout of the GEMMs and every m x n x k of the row GEMM: bit-equal to float64"""
    assert len(_cases(arms, "gemm_")) == len(NS) * len(COUTS) * len(CINS) * len(CIN_EXTS) * 2
    assert len(_cases(arms, "rows_")) == len(ROW_MS) * len(COUTS) * len(CINS)
    _no_errors(arms, "gemm_")
    _no_errors(arms, "rows_")


def test_both_grids_give_the_same_bits(arms):
    for prefix in ("gemm_", "rows_", "pair_ds_", "nonfinite_", "ten_runs_"):
        _arms_bit_equal(arms, prefix)
    _no_errors(arms, "pair_ds_")


def test_nonfinite_values_in_an_odd_chunk_stay_in_their_row(arms):
    assert len(_cases(arms, "nonfinite_")) == 4
    _no_errors(arms, "nonfinite_")


def test_ten_runs_are_bit_identical(arms):
    assert len(_cases(arms, "ten_runs_")) == 3
    _no_errors(arms, "ten_runs_")


def test_local_stage_logits_are_bit_equal_between_the_grids(arms):
    assert len(_cases(arms, "logits_")) == len(LS_BATCHES)
    _no_errors(arms, "logits_")
    _arms_bit_equal(arms, "logits_")
