"""Plain-torch CPU references of the GlobalStage kernels of csrc/be_attn.hip, the cases test_global_kernels_gpu.py runs them at, and the
bounds it holds them to.  Every reference takes a dtype: float64 is the reference, float32 is "the plain float32 evaluation" whose own
distance from float64 shows what float32 arithmetic can reach (test_global_kernels_cpu.py asserts it stays within half of each bound).

Errors are taken per (batch, head) - head_err - or per row - row_err - never over a whole tensor: a wrong head or row group whose
entries are smaller than the tensor's largest would pass a whole-tensor norm.
"""
import functools
import math

import numpy as np
import torch

from be_hip import synth

DH = 16                                                      # head dimension
KB = 32                                                      # keys per block of k_attention
LN2 = math.log(2.0)
EPS = 1e-5

# the project's figures (tests/test_train_gpu.py), applied per head / per row
BOUNDS = dict(out=2e-6, lse=2e-6, grad=5e-6, spike_out=5e-5)
# Cases whose plain float32 evaluation is itself further than HALF a starting bound from float64, per head (nobody had measured these
# figures at L >= 640 per head: 2048 keys and up to 32 heads to take the worst of): the float32 reference's own worst per-head error of
# `out`, as test_global_kernels_cpu.py prints it.  Their bound is four times this figure (the kernel sums in another order and uses
# v_exp_f32); every other case and quantity keeps its starting bound.  The float32 figures depend on the host's matmul and exp (they
# are the same with one thread and with many, but differ between CPU generations by some 10 %): a case is listed when it exceeds half
# the starting bound on any host it was measured on, with the largest figure seen.
F32_REFERENCE_OUT = {
    "nz2_3x6x2048": 1.09e-6, "nz1_4x8x2048": 1.22e-6,                      # starting bound 2e-6 -> 4.36e-6, 4.88e-6
    "spike_last_ragged": 2.87e-5,                                          # starting bound 5e-5 -> 1.15e-4
    "train_2x3x640_p0.0_lv513": 1.11e-6, "train_2x3x640_p0.0_lv544": 1.23e-6, "train_2x3x640_p0.0_lv639": 1.11e-6,   # 2e-6 -> 4.4 .. 4.9e-6
    "train_2x3x640_p0.0_lvNone": 1.06e-6,                                  # 9.33e-7 on one host, 1.06e-6 on another -> 4.24e-6
}


def out_bound(name, spike=False):
    return 4.0 * F32_REFERENCE_OUT[name] if name in F32_REFERENCE_OUT else BOUNDS["spike_out" if spike else "out"]


# ------------------------------------------------------------------------------------------------------------------ error norms
def head_err(got, ref, B, L, H, rows=None):
    """[B, H]: max|got - ref| / max|ref| over each head's [L, 16] block of a [B*L, H*16] tensor (the first `rows` tokens only)."""
    g = got.detach().double().reshape(B, L, H, DH)[:, :rows]
    r = ref.detach().double().reshape(B, L, H, DH)[:, :rows]
    return (g - r).abs().amax(dim=(1, 3)) / r.abs().amax(dim=(1, 3))


def row_err(got, ref, cols=None):
    """[rows]: max|got - ref| / max|ref| over each row (the first `cols` columns only) of a 2-d tensor."""
    g, r = got.detach().double()[:, :cols], ref.detach().double()[:, :cols]
    return (g - r).abs().amax(dim=1) / r.abs().amax(dim=1)


def relmax(got, ref):
    g, r = got.detach().double(), ref.detach().double()
    return float((g - r).abs().max() / r.abs().max())


# ------------------------------------------------------------------------------------------------------------------ attention
def attention_ref(qkv, B, L, H, l_valid=None, mask=None, p=0.0, dtype=torch.float64):
    """softmax(Q K^T / 4) V of qkv [B*L, 3*H*16] per (batch, head), one head at a time (one [L, L] matrix alive); keys >= l_valid carry
    no probability; mask [B*H, L, L] in {0, 1} = the dropout keep decisions (kept probabilities are scaled by 1 / (1 - p), the softmax
    normaliser is the undropped one).  -> out [B*L, H*16], log2-sum-exp of the scaled scores [B*H, L].  Differentiable."""
    D = H * DH
    x = qkv.to(dtype)
    lv = L if l_valid is None else int(l_valid)
    outs, lses = [], []
    for b in range(B):
        xs = x[b * L:(b + 1) * L]
        heads = []
        for h in range(H):
            q = xs[:, h * DH:(h + 1) * DH]
            k = xs[:lv, D + h * DH:D + (h + 1) * DH]
            v = xs[:lv, 2 * D + h * DH:2 * D + (h + 1) * DH]
            s = (q @ k.t()) / 4.0
            m = s.detach().amax(dim=1, keepdim=True)
            e = torch.exp(s - m)
            l = e.sum(dim=1, keepdim=True)
            if mask is not None:
                e = e * (mask[b * H + h][:, :lv].to(dtype) / (1.0 - p))
            heads.append((e @ v) / l)
            lses.append((m + torch.log(l)).squeeze(1) / LN2)
        outs.append(torch.cat(heads, dim=1))
    return torch.cat(outs, dim=0), torch.stack(lses)


def scores_log2(qkv, B, L, H, bh):
    """float64 scores of head bh in the kernel's units (binades): Q K^T / 4 * log2 e, [L, L]"""
    D = H * DH
    b, h = divmod(bh, H)
    xs = qkv.double()[b * L:(b + 1) * L]
    return xs[:, h * DH:(h + 1) * DH] @ xs[:, D + h * DH:D + (h + 1) * DH].t() / 4.0 / LN2


def expected_nz(B, H, L):
    """The documented rule of be_attention_f32: key slices when the query tiles alone leave the chip mostly empty - L >= 2048 and fewer
    than 512 workgroups of 128 queries: four slices up to 256 workgroups, two above."""
    wgs = (L // 128) * B * H
    if L < 2048 or wgs >= 512:
        return 1
    return 4 if wgs <= 256 else 2


def slice_blocks(L, l_valid, nz):
    """[(first key block, one past the last)] of every key slice: the ceil(l_valid / 32) blocks that hold a real key, cut evenly"""
    nblk = -(-(L if l_valid is None else l_valid) // KB)
    return [(nblk * z // nz, nblk * (z + 1) // nz) for z in range(nz)]


def make_qkv(name, B, L, H, spike=None, scale=1.5):
    """float32 [B*L, 3*H*16]; spike = (first token, tokens, tiny first token, tiny tokens): the keys of one range are sixty times longer,
    those of another a hundred times shorter (every batch, every head)"""
    x = synth.hash_normal(31, "gk_qkv_" + name, (B * L, 3 * H * DH)).astype(np.float32) * np.float32(scale)
    if spike is not None:
        D = H * DH
        t0, n, s0, sn = spike
        x = x.reshape(B, L, 3 * D)
        x[:, t0:t0 + n, D:2 * D] *= 60.0
        x[:, s0:s0 + sn, D:2 * D] *= 0.01
        x = x.reshape(B * L, 3 * D)
    return torch.from_numpy(x)


def make_dout(name, B, L, H, l_valid=None):
    """upstream gradient [B*L, H*16], exactly zero on the padding rows (the caller slices the padded output away)"""
    d = torch.from_numpy(synth.hash_normal(32, "gk_dout_" + name, (B * L, H * DH)).astype(np.float32))
    if l_valid is not None:
        d = d * ((torch.arange(B * L) % L) < l_valid)[:, None]
    return d


class InferCase:
    def __init__(self, name, B, H, L, l_valid=None, spike=None, kind="out"):
        self.name, self.B, self.H, self.L, self.l_valid, self.spike, self.kind = name, B, H, L, l_valid, spike, kind
        self.nz = expected_nz(B, H, L)
        self.rows = L if l_valid is None else l_valid

    def __repr__(self):
        return self.name

    def qkv(self):
        return _qkv_of(self)

    def ref(self, dtype=torch.float64):
        """(out, lse) of attention_ref, computed once per dtype and shared: treat as read-only"""
        return _ref_of(self, dtype)

    def bound(self):
        return out_bound(self.name, self.spike is not None)


@functools.lru_cache(maxsize=None)
def _qkv_of(case):
    return make_qkv(case.name, case.B, case.L, case.H, case.spike)


@functools.lru_cache(maxsize=None)
def _ref_of(case, dtype):
    with torch.no_grad():
        return attention_ref(case.qkv(), case.B, case.L, case.H, case.l_valid, dtype=dtype)


# case 1: the key-slice rule on both sides of each threshold
SLICE_CASES = [InferCase("nz4_1x2x2048", 1, 2, 2048), InferCase("nz2_3x6x2048", 3, 6, 2048), InferCase("nz1_4x8x2048", 4, 8, 2048),
               InferCase("nz1_1x2x1920", 1, 2, 1920)]
# case 2: four slices x padded tail: the first legal l_valid, a block-aligned one, one past it, L - 1
RAGGED_CASES = [InferCase(f"ragged_{L}_lv{L - d}", 1, 2, L, l_valid=L - d) for L in (2176, 2048) for d in (127, 96, 95, 1)]
# case 3: the running-maximum path in ONE slice: the third of four (keys 1024..1535), and the last under a padded tail (l_valid 1953:
# 62 key blocks, the last slice is blocks 46..61 = keys 1472..1952)
SPIKE_CASES = [InferCase("spike_slice2", 1, 2, 2048, spike=(1152, 64, 100, 64)),
               InferCase("spike_last_ragged", 1, 2, 2048, l_valid=2048 - 95, spike=(1880, 64, 100, 64))]
SPIKE_SLICE = {"spike_slice2": 2, "spike_last_ragged": 3}
INFER_CASES = SLICE_CASES + RAGGED_CASES + SPIKE_CASES


def slice_rise(case, bh):
    """[nz, L]: per key slice and query, how far (in binades) the slice's largest score sits above the softmax reference the kernel
    fixes from the slice's first block, ceil(max of that block); above 60 the wave takes the running-maximum loop"""
    s = scores_log2(case.qkv(), case.B, case.L, case.H, bh)[:, :case.rows]
    out = []
    for k0, k1 in slice_blocks(case.L, case.l_valid, case.nz):
        first = torch.ceil(s[:, k0 * KB:(k0 + 1) * KB].amax(dim=1))
        out.append(s[:, k0 * KB:min(k1 * KB, case.rows)].amax(dim=1) - first)
    return torch.stack(out)


# case 6: training attention.  (2, 3, 640): 5 query tiles, 20 key blocks, 5 dQ groups, odd head count; (1, 1, 1024): 8 dQ groups
TRAIN_CASES = [(2, 3, 640, p, lv) for p in (0.0, 0.1) for lv in (None, 513, 544, 639)] + [(1, 1, 1024, 0.1, None)]
TRAIN_SEED = 4243


def train_name(case):
    B, H, L, p, lv = case
    return f"train_{B}x{H}x{L}_p{p}_lv{lv}"


def train_ref(qkv, dout, B, L, H, p, l_valid, mask, dtype=torch.float64):
    """autograd reference of the training forward / backward: out, lse, dqkv"""
    x = qkv.to(dtype).requires_grad_(True)
    out, lse = attention_ref(x, B, L, H, l_valid, mask=mask, p=p, dtype=dtype)
    (out * dout.to(dtype)).sum().backward()
    return out.detach(), lse.detach(), x.grad


def keep_mask_from_bits(bits, L):
    """The keep bits k_attention<TRAIN> stores - int16 [BH, L/32, L/32, 64 lanes]; lane (c = lane & 15, g = lane >> 4) of tile (qw, kb)
    holds, in bit 15 - (8 qc + 4 kt + r), the decision of query 32 qw + 16 qc + c, key 32 kb + 16 kt + 4 g + r - as a [BH, L, L] mask"""
    b = (bits.cpu().numpy().astype(np.int32) & 0xffff).astype(np.uint32)
    nb = L // KB
    m = np.zeros((b.shape[0], L, L), np.float32)
    lane = np.arange(64)
    c, g = lane & 15, lane >> 4
    for qc in range(2):
        for kt in range(2):
            for r in range(4):
                qi = KB * np.arange(nb)[:, None, None] + 16 * qc + c[None, None, :]
                ki = KB * np.arange(nb)[None, :, None] + 16 * kt + 4 * g[None, None, :] + r
                m[:, qi, ki] = (b >> (15 - (8 * qc + 4 * kt + r))) & 1
    return torch.from_numpy(m)


# ------------------------------------------------------------------------------------------------------------------ elementwise
def _mix32(x):
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return x


def dropout_keep(n, p, seed, site):
    """The documented counter-based dropout of the elementwise sites: element i is kept iff mix32(i ^ key) >= p 2^32,
    key = mix32(seed + 0x9e3779b9 (site + 1)).  -> float64 {0, 1} [n]"""
    if p <= 0:
        return torch.ones(n, dtype=torch.float64)
    key = _mix32(np.array([(seed + 0x9e3779b9 * (site + 1)) & 0xffffffff], np.uint64))[0]
    thresh = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    keep = _mix32(np.arange(n, dtype=np.uint64) ^ key) >= thresh
    return torch.from_numpy(keep.astype(np.float64))


def attention_keep(B, L, H, p, seed):
    """The documented attention dropout: ONE hash decides the neighbouring keys 2j, 2j + 1 of a query, 16 bits each.  Element
    idx = query L + key of head-batch bh is dropped iff its half (idx & 1) of mix32((idx >> 1) ^ key(seed, bh)) is below p 2^16.
    -> float32 {0, 1} [B*H, L, L]"""
    t16 = np.uint64(int(float(np.float32(p)) * 4294967296.0) >> 16)
    idx = np.arange(L * L, dtype=np.uint64)
    out = np.empty((B * H, L * L), np.float32)
    for bh in range(B * H):
        key = _mix32(np.array([(seed + 0x9e3779b9 * (bh + 1)) & 0xffffffff], np.uint64))[0]
        half = (_mix32((idx >> np.uint64(1)) ^ key) >> (np.uint64(16) * (idx & np.uint64(1)))) & np.uint64(0xffff)
        out[bh] = half >= t16
    return torch.from_numpy(out.reshape(B * H, L, L))


def layernorm_ref(x, res, gamma, beta, eps=EPS, mask=None, p=0.0, dtype=torch.float64):
    """y = LayerNorm(res + dropout(x)) over the last dimension (biased variance about the mean); -> (v = res + dropout(x), y)"""
    v = x.to(dtype)
    if mask is not None:
        v = v * (mask.to(dtype) / (1.0 - p))
    if res is not None:
        v = v + res.to(dtype)
    mean = v.mean(dim=1, keepdim=True)
    c = v - mean
    var = (c * c).mean(dim=1, keepdim=True)
    return v, c / torch.sqrt(var + eps) * gamma.to(dtype) + beta.to(dtype)


def add_pe_ref(x, pe, batches, dtype=torch.float64):
    return (x.to(dtype).reshape(batches, -1) + pe.to(dtype).reshape(1, -1)).reshape(x.shape)


LN_ROWS_CASES = (1, 2, 3, 5, 301)
LN_D_CASES = (64, 128, 192, 256)
LN_TRAIN_ROWS = (1, 31, 33, 1001)
PE_CASES = ((3, 5 * 128), (9, 1024 * 128), (1, 128))
DROPOUT_N = (1, 3, 4, 1023)


def ln_inputs(rows, D, name="ln", plant=True):
    """x, res, gamma, beta, dy (float32).  Planted (inference cases): the LAST row is constant in x + res and in x alone (variance 0: eps decides), the
    FIRST row of a case with at least two rows has mean 1e4 and spread 1 (x carries the offset, res is ordinary)."""
    def hn(k, shape, s=1.0):
        return (s * synth.hash_normal(33, f"gk_{name}_{k}_{rows}_{D}", shape)).astype(np.float32)
    x, res, dy = hn("x", (rows, D)), hn("r", (rows, D)), hn("dy", (rows, D))
    gamma, beta = (1 + hn("g", (D,), 0.3)).astype(np.float32), hn("b", (D,), 0.1)
    if plant:
        x[rows - 1], res[rows - 1] = 0.75, -0.5
        if rows >= 2:
            x[0] += 1e4
    return tuple(torch.from_numpy(a) for a in (x, res, gamma, beta, dy))


def ln_row_bound(v64, y64, gamma, D):
    """[rows] bound on row_err of a LayerNorm output.  BOUNDS['out'] plus what the rounding of the MEAN alone costs: the kernel adds D / 64
    values per lane and six butterfly levels, then divides: at most D / 64 + 6 roundings of a partial sum no larger than D |mean|, so
    |mean' - mean| <= (D / 64 + 6) 2^-24 |mean|, which shifts every y of the row by that times rstd |gamma|.  For ordinary rows
    (|mean| < 1) the term is below 1e-6; for the planted row (mean 1e4, spread 1) it is what decides."""
    mean = v64.mean(dim=1)
    rstd = 1.0 / torch.sqrt(v64.var(dim=1, unbiased=False) + EPS)
    shift = (D // 64 + 6) * 2.0 ** -24 * mean.abs() * rstd * float(gamma.abs().max())
    return BOUNDS["out"] + shift / y64.abs().amax(dim=1)
