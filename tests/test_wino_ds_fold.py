"""The Winograd blocks' 1x1 downsample folded into conv2's transform-domain GEMMs (be_wino.hip, round 14): a 1x1 kernel is a 3x3 with
only the centre tap, its kernel transform is non-zero at 18 of the 40 positions of the 8x5 tiles, and there k_wino_gemm_ps<0, 0, 1>
runs a second K segment over the transform of the block's input: M[z] = V_h[z] U2[z]^T + V_x[z] U_ds[z]^T.

The pack (18 positions, RNE split in block layout); the extended GEMM alone on exact-product operands (every partial sum an fp32 value,
so any order of exact operations gives the same bits: a chunk taken from the wrong segment, position or plane cannot hide in a
tolerance) at one / three / six extension chunks, partial M and N tiles and both layouts; the folded block against float64 beside the
unfolded one, chained and not; bits that depend on neither batch, run nor problem-group count; non-finite inputs; and LocalStage with
the fold (default) against BE_WINO_DS_GEMM=1 in child processes (the knobs are read once per process)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
pytestmark = pytest.mark.gpu
C3 = 1.0 + 2.0 ** -9 + 2.0 ** -17                           # hi, mid and lo all carry bits (test_split_bf16_interleave.py)
NPOS, NLIVE = 40, 18
LIVE = [5 * r + c for r in range(1, 7) for c in range(1, 4)]
# cin -> cmid -> cout (a convolution's input channels are a multiple of 32): 2 / 4 / 6 extension chunks, partial and zero N tiles.
# Where cout is a multiple of 32 a second block can follow: those are run chained too
BLOCKS = [(32, 64, 164), (64, 96, 100), (96, 256, 256), (32, 64, 96)]
NS = (1, 3, 65)                                             # 65 maps = 130 tiles: a partial second M tile
LAYER_TOL = 1.5e-5                                          # the Winograd layer bound of test_hip_parity.py / test_wino_split_bf16.py
KNOBS = ("BE_WINO_DS_GEMM", "BE_WINO_ZGROUPS", "BE_WINO_NO_CHAIN", "BE_WINO_F32", "BE_ROWS_F32", "BE_L0_F32", "BE_C1_F32",
         "BE_NO_CONV_PM", "BE_NO_CONV1_POOL", "BE_WINO_NO_PERSIST", "BE_WINOGRAD")


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    assert n.lib().be_wino_tile_rows() == 6 and n.lib().be_wino_ds_positions() == NLIVE
    return n


def biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def bf16_rne(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32)


def split3(x):
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_rne(r)
    return hi, mid, bf16_rne((r - mid).astype(np.float32))


def block_layout(u, cin):
    """[positions][cout_pad32][cin] fp32 -> the planes as uint16 [positions][N tile][K chunk][plane][row][half][8] (the halves of rows
    8-15, 24-31, ... swapped), rows past cout_pad32 zero"""
    npos, cp32 = u.shape[0], u.shape[1]
    nt, kc = (cp32 + 127) // 128, cin // 16
    full = np.zeros((npos, nt * 128, cin), np.float32)
    full[:, :cp32] = u
    pieces = np.stack([p.view(np.uint32) >> 16 for p in split3(full)]).astype(np.uint16)             # [3][npos][rows][cin]
    e = pieces.reshape(3, npos, nt, 128, kc, 2, 8).transpose(1, 2, 4, 0, 3, 5, 6).copy()
    swap = ((np.arange(128) >> 3) & 1).astype(bool)
    e[:, :, :, :, swap] = e[:, :, :, :, swap][..., ::-1, :]
    return e


def _bn(g, c):
    return tuple(t.to(DEV) for t in (0.5 + torch.rand(c, generator=g), 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g),
                                     0.5 + torch.rand(c, generator=g)))


# ------------------------------------------------------------------------------------------------------------------------------ pack
@pytest.mark.parametrize("cin,cout", [(32, 164), (96, 256), (48, 100)])
def test_centre_tap_transform_has_18_positions_and_the_planes_are_its_rne_split(native, cin, cout):
    g = torch.Generator().manual_seed(1400 + cin + cout)
    w = (torch.randn(cout, cin, generator=g) * float(np.sqrt(2.0 / cin))).to(DEV)
    b = (0.1 * torch.randn(cout, generator=g)).to(DEV)
    bn = _bn(g, cout)
    pd, pb = native.wino_ds_pack(w, b, bn)
    cp = (cout + 31) // 32 * 32
    uds = pd[:NLIVE * cp * cin].cpu().numpy().reshape(NLIVE, cp, cin)
    assert np.all(uds[:, :cout] != 0) and np.all(uds[:, cout:] == 0)            # every live position of every real row carries the tap
    if cin % 32 == 0:                                       # the 3x3 pack (cin % 32) on the centre-tap kernel: the same 18, the same bits
        w3 = torch.zeros(cout, cin, 3, 3, device=DEV)
        w3[:, :, 1, 1] = w
        pw, pb3 = native.wino_pack(w3, b, bn)
        u = pw[:NPOS * cp * cin].cpu().numpy().reshape(NPOS, cp, cin)
        nonzero = [z for z in range(NPOS) if np.any(u[z] != 0)]
        assert nonzero == LIVE and len(nonzero) == 18, nonzero
        dead = [z for z in range(NPOS) if z not in LIVE]
        assert np.all(u[dead] == 0)
        assert np.array_equal(u[LIVE].view(np.uint32), uds.view(np.uint32))
        assert torch.equal(pb, pb3)
    # float64 check of the values: G_rows[:, 1] (x) G_cols[:, 1] times the folded weight
    s = (bn[0] / torch.sqrt(bn[3] + 1e-5)).cpu().double().numpy()
    wf = w.cpu().double().numpy() * s[:, None]
    gr = np.array([0, -2 / 9, 2 / 9, 2 / 90, -2 / 90, 16 / 45, -16 / 45, 0])
    gc = np.array([0, -0.5, 1 / 6, 2 / 6, 0])
    ref = np.stack([gr[z // 5] * gc[z % 5] * wf for z in LIVE])
    assert np.abs(uds[:, :cout] - ref).max() <= 4e-7 * np.abs(ref).max()
    planes = pd[NLIVE * cp * cin:].cpu().numpy().view(np.uint16)
    e = block_layout(uds, cin)
    assert planes.size == e.size and np.array_equal(planes.reshape(e.shape), e)


# ------------------------------------------------------------------------------------------------- the extended GEMM, exact products
def _three_piece(shape, rng):
    v = rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float64), size=shape) * C3
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v


def _sparse(shape, nnz, rng):
    """[..., k] in {0, +-1, +-2} with at most nnz non-zeros along k"""
    v = np.zeros(shape)
    idx = rng.integers(0, shape[-1], size=shape[:-1] + (nnz,))
    np.put_along_axis(v, idx, rng.choice(np.array([-2, -1, 1, 2], np.float64), size=idx.shape), axis=-1)
    return v


def _packed_from_u(native, u, cout, cin):
    """a packed buffer of the GEMMs from transform-domain weights u [positions][cout][cin] given directly (no kernel transform): the
    fp32 part (which the split-bf16 GEMMs do not read) zero, then each position's planes (gemm_rows_bf6_pack: one position's layout)"""
    cp = (cout + 31) // 32 * 32
    planes = []
    for z in range(u.shape[0]):
        pw = torch.zeros(cp, cin)
        pw[:cout] = torch.as_tensor(u[z], dtype=torch.float32)
        planes.append(native.gemm_rows_bf6_pack(pw.reshape(-1).to(DEV), cout, cin))
    return torch.cat([torch.zeros(u.shape[0] * cp * cin, device=DEV)] + planes)


@pytest.mark.parametrize("cin_ext", [16, 48, 96])
@pytest.mark.parametrize("cmid", [32, 64])
def test_extended_gemm_exact_products_equal_two_plain_gemms(native, cin_ext, cmid):
    rng = np.random.default_rng(1410 + cin_ext + cmid)
    nmax = max(NS)
    v = _three_piece((NPOS, 2 * nmax, cmid), rng)
    vx = _three_piece((NPOS, 2 * nmax, cin_ext), rng)
    for cout in (100, 164):
        u2 = _sparse((NPOS, cout, cmid), 10, rng)
        uds = _sparse((NLIVE, cout, cin_ext), 10, rng)
        uds_all = np.zeros((NPOS, cout, cin_ext))
        uds_all[LIVE] = uds
        assert (np.abs(v) @ np.abs(u2).transpose(0, 2, 1) + np.abs(vx) @ np.abs(uds_all).transpose(0, 2, 1)).max() < 128.0
        ref = v @ u2.transpose(0, 2, 1) + vx @ uds_all.transpose(0, 2, 1)                    # [40][tiles][cout], exact in float64
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
        pw2 = _packed_from_u(native, u2, cout, cmid)
        pds = _packed_from_u(native, uds, cout, cin_ext)
        pds_all = _packed_from_u(native, uds_all, cout, cin_ext)
        for n in NS:
            for tm in (False, True):
                lay = (lambda a: np.ascontiguousarray(a.transpose(1, 0, 2))) if tm else (lambda a: np.ascontiguousarray(a))
                vd = torch.from_numpy(lay(v[:, :2 * n]).astype(np.float32)).to(DEV)
                vxn = vx[:, :2 * n].astype(np.float32)
                vxz = vxn.copy()
                vxz[[z for z in range(NPOS) if z not in LIVE]] = 0.0
                vxp = vxn.copy()                                 # positions without extension: poisoned, must never be read
                vxp[[z for z in range(NPOS) if z not in LIVE]] = np.nan
                ext = native.wino_gemms_ext(vd, pw2, n, cmid, cout, torch.from_numpy(lay(vxp)).to(DEV), pds, cin_ext, tile_major=tm)
                plain = native.wino_gemms_ext(vd, pw2, n, cmid, cout, tile_major=tm)
                second = native.wino_gemms_ext(torch.from_numpy(lay(vxz)).to(DEV), pds_all, n, cin_ext, cout, tile_major=tm)
                what = (cin_ext, cmid, cout, n, tm)
                assert biteq(ext, plain + second), what
                e, p = (t.permute(1, 0, 2) if tm else t for t in (ext, plain))
                dead = [z for z in range(NPOS) if z not in LIVE]
                assert biteq(e[dead], p[dead]), what
                assert np.array_equal(e.cpu().numpy(), ref[:, :2 * n].astype(np.float32)), what


# ------------------------------------------------------------------------------------------------------------------ the folded block
_BLOCKS = {}


def _block(native, cin, cm, c):
    """One residual block cin -> cm -> c (+ 1x1 downsample cin -> c), packed for both forms, and (c % 32 == 0) a following block
    c -> c -> c."""
    if (cin, cm, c) not in _BLOCKS:
        g = torch.Generator().manual_seed(1420 + cin + 3 * c + 5 * cm)
        t = {}
        convs = [("c1", cm, cin, 3), ("c2", c, cm, 3), ("ds", c, cin, 1)]
        if c % 32 == 0:
            convs += [("d1", c, c, 3), ("d2", c, c, 3), ("dds", c, c, 1)]
        for name, co, ci, k in convs:
            t[name] = (torch.randn(co, ci, k, k, generator=g) * float(np.sqrt(2.0 / (k * k * ci))), 0.1 * torch.randn(co, generator=g))
        p = {"t": t}
        for name in [k for k in t if k in ("c1", "c2", "d1", "d2")]:
            p[name] = native.wino_pack(t[name][0].to(DEV), t[name][1].to(DEV))
        for name, conv2 in [(a, b) for a, b in (("ds", "c2"), ("dds", "d2")) if a in t]:
            w, b = t[name]
            co, ci = w.shape[:2]
            p[name] = native.wino_ds_pack(w.reshape(co, ci).to(DEV), b.to(DEV))
            p[conv2 + "b"] = p[conv2][1] + p[name][1]                                # the downsample's bias joins conv2's
            pw = torch.zeros((co + 31) // 32 * 32, ci)
            pw[:co] = w.reshape(co, ci)
            p[name + "_rows"] = native.gemm_rows_bf6_pack(pw.reshape(-1).to(DEV), co, ci)
        _BLOCKS[(cin, cm, c)] = p
    return _BLOCKS[(cin, cm, c)]


def _act64(v, act):
    if act == 1:
        return v * torch.tanh(torch.log(1 + torch.sigmoid(v)))
    return v.clamp_min(0) if act == 2 else v


def _ref64(t, x, act2, names=("c1", "c2", "ds")):
    F = torch.nn.functional
    xd = x.cpu().double().permute(0, 3, 1, 2)
    (w1, b1), (w2, b2), (wd, bd) = (tuple(a.double() for a in t[k]) for k in names)
    h = _act64(F.conv2d(xd, w1, b1, padding=1), 1)
    return _act64(F.conv2d(h, w2, b2, padding=1) + F.conv2d(xd, wd, bd), act2).permute(0, 2, 3, 1)


def _unfolded(native, p, x, cm, c, act2):
    r = native.gemm_rows_bf6(x.reshape(-1, x.shape[-1]), p["ds_rows"], c).reshape(x.shape[0], 6, 6, c)
    return native.wino_conv3x3_pair(x, *p["c1"], cm, p["c2"][0], p["c2b"], c, act1=1, act2=act2, residual=r)[0]


def _folded(native, p, x, cm, c, **kw):
    return native.wino_conv3x3_pair_ds(x, *p["c1"], cm, p["c2"][0], p["c2b"], p["ds"][0], c, **kw)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("cin,cm,c", BLOCKS)
def test_folded_block_vs_float64_chained_and_not(native, cin, cm, c, n):
    p = _block(native, cin, cm, c)
    g = torch.Generator().manual_seed(1430 + n + c)
    x = torch.randn(n, 6, 6, cin, generator=g).to(DEV)
    lib = native.lib()
    for act in (0, 1, 2):
        ref = _ref64(p["t"], x, act)
        y, _ = _folded(native, p, x, cm, c, act2=act)
        e_f, e_u = relmax(y.cpu(), ref), relmax(_unfolded(native, p, x, cm, c, act).cpu(), ref)
        print(f"block {cin}->{cm}->{c} n={n} act={act}: folded {e_f:.2e}  unfolded {e_u:.2e}  (bound {LAYER_TOL})")
        assert e_f <= LAYER_TOL, (cin, cm, c, n, act, e_f, e_u)
        if c % 32:
            continue
        # chained: the block leaves the next block's input transform in the workspace; the next block (folded too) is handed no map
        nxt = lambda xin, **kw: native.wino_conv3x3_pair_ds(xin, *p["d1"], c, p["d2"][0], p["d2b"], p["dds"][0], c, **kw)[0]
        need = max(lib.be_wino_pair_ds_workspace_floats(n, cin, cm, c), lib.be_wino_pair_ds_workspace_floats(n, c, c, c))
        ws = torch.full((need,), float("nan"), dtype=torch.float32, device=DEV)
        y1, _ = _folded(native, p, x, cm, c, act2=act, workspace=ws, next_cmid=c)
        z1 = nxt(None, workspace=ws, x_in_v=True, cin=c, n=n)
        assert biteq(y1, y), (cin, cm, c, n, act)
        z = nxt(y)
        assert biteq(z1, z), (cin, cm, c, n, act)
        e_z = relmax(z.cpu(), _ref64(p["t"], y, 1, ("d1", "d2", "dds")))       # the following block on the map it was given
        print(f"   following block {c}->{c}->{c}: folded {e_z:.2e}")
        assert e_z <= LAYER_TOL
        ws.fill_(float("nan"))                                   # the same chain without the store of y
        none, _ = _folded(native, p, x, cm, c, act2=act, workspace=ws, next_cmid=c, store_y=False)
        assert none is None and biteq(nxt(None, workspace=ws, x_in_v=True, cin=c, n=n), z), (cin, cm, c, n, act)


def _fold_outputs():
    """the folded block 96 -> 256 on the first n maps of one seeded batch of 130 (child processes import this)"""
    from be_hip import native
    native.lib()
    cin, c = 96, 256
    p = _block(native, cin, c, c)
    x = torch.randn(130, 6, 6, cin, generator=torch.Generator().manual_seed(1440)).to(DEV)
    return {f"n{n}": _folded(native, p, x[:n].contiguous(), c, c)[0].cpu().numpy() for n in NS + (130,)}


_CHILD = r'''
import os, sys
import numpy as np
sys.path[:0] = [os.environ["BE_ROOT"], os.path.join(os.environ["BE_ROOT"], "blurry-edges_amd"), os.path.join(os.environ["BE_ROOT"], "tests")]
import test_wino_ds_fold as t
np.savez(os.environ["BE_OUT"], **getattr(t, os.environ["BE_WHAT"])())
'''


def _child(d, name, what, **knobs):
    env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, name + ".npz"), BE_WHAT=what)
    for k in KNOBS:
        env.pop(k, None)
    env.update(knobs)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-4000:])
    return dict(np.load(os.path.join(d, name + ".npz")))


def test_folded_block_bits_depend_on_neither_batch_nor_run_nor_group_count(native):
    cin, c = 96, 256
    p = _block(native, cin, c, c)
    got = _fold_outputs()
    for n in NS:
        assert got[f"n{n}"].tobytes() == got["n130"][:n].tobytes(), n
    x = torch.randn(130, 6, 6, cin, generator=torch.Generator().manual_seed(1440)).to(DEV)
    ws = None
    for _ in range(10):
        y, ws = _folded(native, p, x, c, c, workspace=ws)
        assert y.cpu().numpy().tobytes() == got["n130"].tobytes()
    with tempfile.TemporaryDirectory() as d:                    # 3 does not divide 40 (a short last group), 8 does
        for zg in ("3", "8"):
            other = _child(d, "zg" + zg, "_fold_outputs", BE_WINO_ZGROUPS=zg)
            for k, v in got.items():
                assert other[k].tobytes() == v.tobytes(), (zg, k)


def test_nonfinite_input_of_one_map_stays_in_that_map(native):
    cin, cm, c = 64, 96, 100
    p = _block(native, cin, cm, c)
    g = torch.Generator().manual_seed(1450)
    x = torch.randn(5, 6, 6, cin, generator=g)
    clean = _folded(native, p, x.to(DEV), cm, c)[0]
    for bad, ch in ((float("nan"), 3), (float("inf"), 40), (float("-inf"), 63)):      # channel 40: the extension's third chunk
        xb = x.clone()
        xb[2, 3, 2, ch] = bad
        y = _folded(native, p, xb.to(DEV), cm, c)[0]
        keep = [0, 1, 3, 4]
        assert biteq(y[keep], clean[keep]), bad
        assert not bool(torch.isfinite(y[2]).all()), bad


# --------------------------------------------------------------------------------------------------------------------- whole LocalStage
LS_BATCHES = (3, 700, 4200)                                 # plane-major, and tile-major buffers (>= 1024 maps)
LS_CHUNKS = (0, 1000, 4096)


def _logits():
    """LocalStage logits (Winograd path) of the first n patches of one seeded batch for every batch size and chunk, and the profiler's
    count of split-bf16 row GEMM launches (kernel id 7) in one 65-patch forward."""
    import models
    from be_hip import native, synth
    m = models.LocalStage()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.local_stage_state_dict().items()})
    m = m.to(DEV).eval()
    assert m.winograd is True
    x = torch.from_numpy(np.asarray(synth.uniform_patches(max(LS_BATCHES), name="wino_ds_fold"), dtype=np.float32)).to(DEV)
    out = {}
    with torch.no_grad():
        for n in LS_BATCHES:
            for chunk in LS_CHUNKS:
                m.chunk = chunk
                out[f"n{n}_c{chunk}"] = m(x[:n].contiguous()).cpu().numpy().copy()
        m.chunk = 0
        native.profile_enable(256)
        native.profile_reset()
        m(x[:65].contiguous())
        torch.cuda.synchronize()
        ids = [r[0] for r in native.profile_read(256)]
    out["launches"] = np.array([ids.count(7), ids.count(6), ids.count(8)])
    return out


def test_local_stage_with_the_fold_against_the_separate_downsample(native):
    with tempfile.TemporaryDirectory() as d:                    # one after the other
        arms = {"default": _child(d, "default", "_logits"), "ds_gemm": _child(d, "ds_gemm", "_logits", BE_WINO_DS_GEMM="1")}
    print({k: v["launches"].tolist() for k, v in arms.items()})
    full = arms["default"][f"n{max(LS_BATCHES)}_c0"]
    assert np.isfinite(full).all()
    for n in LS_BATCHES:                                        # the default arm is batch- and chunk-independent
        for chunk in LS_CHUNKS:
            assert arms["default"][f"n{n}_c{chunk}"].tobytes() == full[:n].tobytes(), (n, chunk)
    new, old = full, arms["ds_gemm"][f"n{max(LS_BATCHES)}_c0"]
    assert new.tobytes() != old.tobytes()                       # the knob reaches the kernels
    e = relmax(new, old)
    print(f"default (folded) vs BE_WINO_DS_GEMM=1 logits: relmax {e:.2e}")
    assert e <= 1e-5                                            # the bound tests/test_rows_split_bf16.py holds between its arms
    # row GEMM launches per forward: fc.1 alone with the fold, fc.1 and the three downsamples under the knob; six Winograd GEMM
    # launches and seven transform launches either way
    assert arms["default"]["launches"].tolist() == [1, 6, 7], arms["default"]["launches"]
    assert arms["ds_gemm"]["launches"].tolist() == [4, 6, 7], arms["ds_gemm"]["launches"]
