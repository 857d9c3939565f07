"""Adversarial inputs for the attention kernels (csrc/attention_kernels.hip), the float64 statement of the operation they are judged
against, and the list of kernel instantiations that ``ops`` can reach.  No tests here and nothing that needs a GPU: the builders make
their data with a CPU generator (so the CPU test of the builders sees the very tensors the GPU tests run) and move it to ``device``.

Every builder takes ``(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu")`` and returns ``q, k, v`` ([B, N, H * head_dim], 16-bit).  The
rows a builder plants sit at the fixed places ``WHERE`` names, so a test can pick them out again.  A builder asserts the property
its docstring states, in float64 on the tensors it returns: data that lost its property (another seed, another shape) stops the
test that asked for it instead of quietly checking nothing.
"""
import math
from dataclasses import dataclass

import torch

TILE = 64                      # keys per tile of every multi-tile kernel (KT in attention_kernels.hip)
BLOCK = 32                     # keys per block of the one-pass kernels (small-KV, IP)
LN2 = 0.6931471805599453
LOG2E = 1.4426950408889634
CREEP_STEP = 0.35              # natural units per tile = 0.505 in log2 units (test_flash_attention_deferred_rescale_branches)

# (batch, head, query row) of every planted row; a negative batch counts from the end, heads are taken modulo H
WHERE = {
    "late_outlier": (0, 0, 5),
    "uniform_row": (-1, None, 7),      # q = 0 in every head of that row
    "first_tile_max": (0, 1, 17),
    "creeping_max": (0, 1, 3),
    "all_negative": (0, 2, 9),
}
MIN_NQ = 18                    # the planted rows above need query rows 3 .. 17


# ---- float64 reference -----------------------------------------------------------------------------------------------------------
def _heads64(t, heads):
    B, N, HD = t.shape
    return t.double().reshape(B, N, heads, HD // heads).transpose(1, 2)


def attention_ref64(q, k, v, heads, scale):
    """softmax(scale * q k^T) v per head in float64, on the 16-bit values as given (any strides).  ``scale``: head_dim ** -0.5, or
    ln 2 for exponent-domain queries (v_path 6)."""
    B, Nq, HD = q.shape
    qf, kf, vf = (_heads64(t, heads) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) * scale
    return (torch.softmax(s, dim=-1) @ vf).transpose(1, 2).reshape(B, Nq, HD)


def ip_ref64(q, k, v, heads, n_text, ip_scale):
    """IP-Adapter decoupled cross attention in float64: the first ``n_text`` rows of k / v are one softmax, the rows behind them a
    second one, out = text + ip_scale * image (head_dim ** -0.5 in both)."""
    scale = (q.shape[-1] // heads) ** -0.5
    return (attention_ref64(q, k[:, :n_text], v[:, :n_text], heads, scale)
            + ip_scale * attention_ref64(q, k[:, n_text:], v[:, n_text:], heads, scale))


def scores64(q, k, heads, b, h, row, scale):
    """[Nk] float64 scores (after the scale) of one query row of one head."""
    hd = q.shape[-1] // heads
    sl = slice(h * hd, (h + 1) * hd)
    return (k[b, :, sl].double() @ q[b, row, sl].double()) * scale


def exp2_q(q, head_dim=64):
    """Exponent-domain queries for v_path 6: q * (softmax scale * log2 e), rounded once to the 16-bit type.  The operation on them
    is the softmax to base 2, i.e. ``scale = LN2`` in the reference."""
    return (q.float() * (head_dim ** -0.5 * LOG2E)).to(q.dtype)


# ---- the kernel instantiations ops can reach -----------------------------------------------------------------------------------
@dataclass(frozen=True)
class Target:
    name: str            # "<family>/<instantiation>": fwd/0-3, pipe/4-10, smallkv/NKB, ip/NKB, gen/DH
    family: str          # the __global__ template in attention_kernels.hip
    head_dim: int
    nk_min: int          # keys (text keys for ip) this instantiation takes ...
    nk_max: int          # ... up to here (None: no limit)
    online: bool         # multi-tile online softmax (else one pass over <= 160 keys)
    v_path: int = None   # what ops.flash_attention is given (None: the head dim or the entry point selects the kernel)
    exp2: bool = False   # takes exponent-domain queries

    @property
    def ip(self):
        return self.family == "k_flash_attn_ip"

    @property
    def scale(self):
        return LN2 if self.exp2 else self.head_dim ** -0.5

    def takes(self, nk):
        return nk >= self.nk_min and (self.nk_max is None or nk <= self.nk_max)

    @property
    def ragged_nk(self):
        """smallest key count with more than one block / tile and a ragged last one"""
        n = max(self.nk_min, (TILE if self.online else BLOCK) + 1)
        while n % (TILE if self.online else BLOCK) == 0:
            n += 1
        assert self.takes(n)
        return n

    def prep_q(self, q):
        """the queries this target is given (and judged on)"""
        return exp2_q(q, self.head_dim) if self.exp2 else q

    def run(self, ops, q, k, v, heads, n_text=None, ip_scale=None):
        """``q`` as ``prep_q`` returned it"""
        if self.ip:
            return ops.flash_attention_ip(q, k, v, heads, n_text, ip_scale)
        if self.v_path is None:
            return ops.flash_attention(q, k, v, heads)
        return ops.flash_attention(q, k, v, heads, v_path=self.v_path, prescaled=self.exp2)

    def ref64(self, q, k, v, heads, n_text=None, ip_scale=None):
        if self.ip:
            return ip_ref64(q, k, v, heads, n_text, ip_scale)
        return attention_ref64(q, k, v, heads, self.scale)


def _targets():
    from elasticdiffusion_official_amd import ops
    assert ops.SMALLKV_MAX_KEYS == 5 * BLOCK and ops.IP_MAX_TEXT_KEYS == 5 * BLOCK and ops.IP_MAX_IMAGE_KEYS == BLOCK
    out = [Target(f"fwd/{p}", "k_flash_attn_fwd", 64, 1, None, True, p) for p in (0, 1, 2, 3)]
    # 4 / 5 run from one key on; ed_flash_attention refuses 7 / 9 / 10 below one full tile, ops.flash_prescale hands out
    # exponent-domain queries (6) from two full tiles on (ops._pipe_fits)
    pipe_min = {4: 1, 5: 1, 6: 2 * TILE, 7: TILE, 9: TILE, 10: TILE}
    assert not ops._pipe_fits(2 * TILE - 1, 64) and ops._pipe_fits(2 * TILE, 64)
    out += [Target(f"pipe/{p}", "k_flash_attn_pipe", 64, pipe_min[p], None, True, p, exp2=p == 6) for p in (4, 5, 6, 7, 9, 10)]
    classes = ((2, 1, 2 * BLOCK), (3, 2 * BLOCK + 1, 3 * BLOCK), (5, 3 * BLOCK + 1, ops.SMALLKV_MAX_KEYS))
    out += [Target(f"smallkv/{nkb}", "k_flash_attn_smallkv", 64, lo, hi, False, 8) for nkb, lo, hi in classes]
    out += [Target(f"ip/{nkb}", "k_flash_attn_ip", 64, lo, min(hi, ops.IP_MAX_TEXT_KEYS), False) for nkb, lo, hi in classes]
    out += [Target(f"gen/{hd}", "k_flash_attn_gen", hd, 1, None, True) for hd in ops.FLASH_HEAD_DIMS if hd != 64]
    return tuple(out)


TARGETS = _targets()
BY_NAME = {t.name: t for t in TARGETS}
ONLINE = tuple(t for t in TARGETS if t.online)
ONE_PASS = tuple(t for t in TARGETS if not t.online)


def one_pass_target(kind, n):
    """the small-KV (``kind`` "smallkv") or IP ("ip") instantiation that takes ``n`` (text) keys"""
    return next(t for t in ONE_PASS if t.name.startswith(kind + "/") and t.takes(n))


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _base(dtype, head_dim, B, H, Nq, Nk, seed, sq=1.0, sk=1.0, sv=1.0):
    """unit Gaussians on the CPU: scores ~ N(0, sq * sk) after the scale"""
    g = _gen(seed)
    return tuple(_randn(g, B, n, H * head_dim).mul(s).to(dtype) for n, s in ((Nq, sq), (Nk, sk), (Nk, sv)))


def _pattern(head_dim, seed):
    """a fixed +-1 pattern (exact in every format)"""
    return torch.where(_randn(_gen(1000 + seed), head_dim) >= 0, 1.0, -1.0)


def _at(name, B, H):
    b, h, row = WHERE[name]
    return b % B, (None if h is None else h % H), row


def _hs(h, hd):
    return slice(h * hd, (h + 1) * hd)


def outlier_key(Nk):
    """key index late_outlier plants: inside the LAST FULL 64-key tile (the last key where there is no full tile)"""
    return (Nk // TILE - 1) * TILE + 24 if Nk >= TILE else Nk - 1


def first_key(Nk):
    """key index first_tile_max plants (tile 0)"""
    return min(5, Nk - 1)


def creeping_keys(Nk):
    """one key per tile, the ragged one included"""
    return [min(TILE * t + 40, Nk - 1) for t in range((Nk + TILE - 1) // TILE)]


def _plant_outlier(q, k, heads, seed):
    B, Nq, HD = q.shape
    hd, Nk = HD // heads, k.shape[1]
    b, h, row = _at("late_outlier", B, heads)
    pat = _pattern(hd, seed)
    # q = 8 * pattern, k = c * pattern: score = sqrt(hd) * 8 c = 180; every other key scores N(0, 8^2) against this query, and
    # this key scores N(0, c^2), c <= 3.6, against every other query
    q[b, row, _hs(h, hd)] = (8.0 * pat).to(q.dtype)
    k[b, outlier_key(Nk), _hs(h, hd)] = (180.0 / (8.0 * math.sqrt(hd)) * pat).to(k.dtype)


def _plant_first(q, k, heads):
    B, Nq, HD = q.shape
    hd, Nk = HD // heads, k.shape[1]
    b, h, row = _at("first_tile_max", B, heads)
    qr = q[b, row, _hs(h, hd)].float()
    k[b, first_key(Nk), _hs(h, hd)] = (qr.sign() * (25.0 * math.sqrt(hd) / float(qr.abs().sum()))).to(k.dtype)   # score 25


def _plant_creeping(q, k, heads, step=CREEP_STEP):
    """after every other plant in that head: the ladder starts above whatever the row already scores"""
    B, Nq, HD = q.shape
    hd, Nk = HD // heads, k.shape[1]
    b, h, row = _at("creeping_max", B, heads)
    qr = q[b, row, _hs(h, hd)].double()
    base = float(scores64(q, k, heads, b, h, row, hd ** -0.5).max()) + 0.5
    for t, key in enumerate(creeping_keys(Nk)):
        k[b, key, _hs(h, hd)] = (qr * ((base + step * t) * math.sqrt(hd) / float(qr.pow(2).sum()))).to(k.dtype)


def _plant_negative(q, k, heads, seed):
    B, Nq, HD = q.shape
    hd = HD // heads
    b, h, row = _at("all_negative", B, heads)
    w = _pattern(hd, seed + 1)
    # every key of the head moves by d w and the query is -2 w: score = -2 d sqrt(hd) - 2 w.k0 / sqrt(hd) = -40 + N(0, 2^2).  The
    # other queries of the head see one constant added to all their scores, which a softmax does not notice
    k[b, :, _hs(h, hd)] = (k[b, :, _hs(h, hd)].float() + (20.0 / math.sqrt(hd)) * w).to(k.dtype)
    q[b, row, _hs(h, hd)] = (-2.0 * w).to(q.dtype)


def _plant_uniform(q, heads):
    b, _, row = _at("uniform_row", q.shape[0], heads)
    q[b, row] = 0


def margin(s, key):
    """score of ``key`` minus the largest other score (inf when there is no other key)"""
    rest = torch.cat([s[:key], s[key + 1:]])
    return float(s[key] - rest.max()) if rest.numel() else float("inf")


def tile_maxima(s):
    return [float(s[a:a + TILE].max()) for a in range(0, s.numel(), TILE)]


def _check(name, q, k, v, heads, step=CREEP_STEP):
    """the stated property, in float64 on the 16-bit tensors (for v_path 6 the test checks again on the converted q)"""
    B, Nq, HD = q.shape
    hd, Nk = HD // heads, k.shape[1]
    b, h, row = _at(name, B, heads)
    if name == "uniform_row":
        assert not bool(q[b, row].any())
        return
    s = scores64(q, k, heads, b, h, row, hd ** -0.5)
    if name == "late_outlier":
        assert margin(s, outlier_key(Nk)) > 100.0, margin(s, outlier_key(Nk))
    elif name == "first_tile_max":
        assert int(s.argmax()) == first_key(Nk) and margin(s, first_key(Nk)) > 5.0, (int(s.argmax()), margin(s, first_key(Nk)))
    elif name == "creeping_max":
        keys, mx = creeping_keys(Nk), tile_maxima(s)
        assert [int(s[TILE * t:TILE * (t + 1)].argmax()) + TILE * t for t in range(len(keys))] == keys
        assert all(0.8 * step < b_ - a_ < 1.2 * step for a_, b_ in zip(mx, mx[1:])), mx
    elif name == "all_negative":
        assert -60.0 <= float(s.min()) and float(s.max()) <= -20.0, (float(s.min()), float(s.max()))


def _finish(names, q, k, v, heads, device, **kw):
    for n in names:
        _check(n, q, k, v, heads, **kw)
    return q.to(device), k.to(device), v.to(device)


def _need(Nq, H=1, heads_needed=1):
    assert Nq >= MIN_NQ, f"the planted rows need Nq >= {MIN_NQ}"
    assert H >= heads_needed, f"these rows need {heads_needed} heads to stay apart"


def gaussian(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu"):
    """test_flash_attention's data: q, k ~ 1.5 N(0, 1), v ~ N(0, 1); scores ~ N(0, 2.25).  No planted row."""
    return tuple(t.to(device) for t in _base(dtype, head_dim, B, H, Nq, Nk, seed, 1.5, 1.5, 1.0))


def late_outlier(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu"):
    """Query WHERE["late_outlier"] scores 180 (natural units, after the scale) against key ``outlier_key(Nk)`` in the LAST FULL
    64-key tile and N(0, 8^2) against all others: a margin > 100.  The running maximum jumps by > 100 in a late tile and every
    earlier numerator must be rescaled to nothing; the output row is that key's V row."""
    _need(Nq)
    q, k, v = _base(dtype, head_dim, B, H, Nq, Nk, seed)
    _plant_outlier(q, k, H, seed)
    return _finish(["late_outlier"], q, k, v, H, device)


def creeping_max(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu", step=CREEP_STEP):
    """Query WHERE["creeping_max"]: key ``creeping_keys(Nk)[t]`` is the best of tile t and scores base + 0.35 t (natural units; 0.505
    per tile in log2 units), base = 0.5 above every other score of the row.  test_flash_attention_deferred_rescale_branches' ladder
    for any head dim: k = q * s sqrt(hd) / |q|^2 scores s after the 1 / sqrt(hd).  The maximum moves every tile by less than any
    deferred-rescale threshold, and by more than it in total from 12 tiles on."""
    _need(Nq)
    q, k, v = _base(dtype, head_dim, B, H, Nq, Nk, seed)
    _plant_creeping(q, k, H, step)
    return _finish(["creeping_max"], q, k, v, H, device, step=step)


def first_tile_max(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu"):
    """Query WHERE["first_tile_max"] scores 25 against key ``first_key(Nk)`` of tile 0 and N(0, 1) against the rest: the running
    maximum is final after the first tile and no later tile may move it."""
    _need(Nq)
    q, k, v = _base(dtype, head_dim, B, H, Nq, Nk, seed)
    _plant_first(q, k, H)
    return _finish(["first_tile_max"], q, k, v, H, device)


def uniform_row(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu"):
    """Query row WHERE["uniform_row"] is zero in every head: all scores equal, the output row is the mean of V over the keys."""
    _need(Nq)
    q, k, v = _base(dtype, head_dim, B, H, Nq, Nk, seed)
    _plant_uniform(q, H)
    return _finish(["uniform_row"], q, k, v, H, device)


def all_negative(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu"):
    """Every score of query WHERE["all_negative"] lies in [-60, -20] (-40 + N(0, 2^2)): a running maximum that starts from 0
    instead of -inf, or a masked score set to 0 instead of -inf, takes the whole row."""
    _need(Nq)
    q, k, v = _base(dtype, head_dim, B, H, Nq, Nk, seed)
    _plant_negative(q, k, H, seed)
    return _finish(["all_negative"], q, k, v, H, device)


def planted_rows(creeping=True):
    return ["late_outlier", "first_tile_max"] + (["creeping_max"] if creeping else []) + ["uniform_row", "all_negative"]


def combined(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu", creeping=True):
    """late_outlier and uniform_row (head 0), first_tile_max and creeping_max (head 1; ``creeping=False`` for the one-pass kernels)
    and all_negative (head 2) in one tensor, each with the property its own builder states."""
    _need(Nq, H, 3)
    q, k, v = _base(dtype, head_dim, B, H, Nq, Nk, seed)
    _plant_outlier(q, k, H, seed)
    _plant_first(q, k, H)
    _plant_negative(q, k, H, seed)
    if creeping:
        _plant_creeping(q, k, H)     # last in its head: the ladder starts above first_tile_max's key
    _plant_uniform(q, H)
    return _finish(planted_rows(creeping), q, k, v, H, device)


V_LARGE = 3.0e4


def large_v(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu"):
    """fp16 only: v ~ 1.2e4 N(0, 1) clamped to +-3e4 (both ends occur), with uniform_row's row (output = mean of V) and late_outlier's
    row (output = one V row).  Every output is a convex combination of V rows, so it must stay finite and below 3e4."""
    assert dtype == torch.float16
    _need(Nq)
    q, k, v = _base(dtype, head_dim, B, H, Nq, Nk, seed)
    v = v.float().mul(1.2e4).clamp(-V_LARGE, V_LARGE)
    v[0, 0, 0], v[0, 0, 1] = V_LARGE, -V_LARGE
    v = v.to(dtype)
    _plant_outlier(q, k, H, seed)
    _plant_uniform(q, H)
    assert float(v.float().abs().max()) == V_LARGE
    return _finish(["late_outlier", "uniform_row"], q, k, v, H, device)


def fused_columns(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu"):
    """gaussian's values; q / k / v are column slices of one [B, N, 3 * inner] tensor when Nq == Nk (a fused QKV projection), else
    q is its own tensor and k | v are the halves of one [B, Nk, 2 * inner] (a fused KV projection): token stride 3 or 2 * inner."""
    q, k, v = gaussian(dtype, head_dim, B, H, Nq, Nk, seed)
    inner = H * head_dim
    if Nq == Nk:
        qkv = torch.cat([q, k, v], dim=-1).to(device)
        return qkv[..., :inner], qkv[..., inner:2 * inner], qkv[..., 2 * inner:]
    kv = torch.cat([k, v], dim=-1).to(device)
    return q.to(device), kv[..., :inner], kv[..., inner:]


def every_second_batch(dtype, head_dim, B, H, Nq, Nk, seed, device="cpu"):
    """gaussian's values; every operand is ``[::2]`` of a tensor with 2 B entries (batch stride twice the entry's size), the odd
    entries holding other finite data."""
    big = gaussian(dtype, head_dim, 2 * B, H, Nq, Nk, seed, device)
    return tuple(t[::2] for t in big)


# ---- layouts around K and V ------------------------------------------------------------------------------------------------------
def _rehost(t, front_rows, behind_rows, fill):
    B, N, HD = t.shape
    per = N + behind_rows
    pool = torch.empty(front_rows * HD + B * per * HD, dtype=t.dtype, device=t.device)
    fill(pool)
    view = pool.as_strided((B, N, HD), (per * HD, HD, 1), front_rows * HD)
    view.copy_(t)
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 0 and view.stride(1) % 8 == 0
    return view


def poisoned(k, v, front_rows, gap_rows):
    """K and V re-hosted, one allocation each, with NaN (Inf at every second element) in ``front_rows`` rows in front of batch 0
    and in ``gap_rows`` rows behind EVERY batch entry, the last included: views with stride(0) = (Nk + gap_rows) * stride(1), 16-byte
    aligned bases and strides that are multiples of 8.  A load of a row before 0 or past Nk of ANY batch entry turns the output
    non-finite (0 * NaN and 0 * Inf are NaN)."""
    def fill(pool):
        pool.fill_(float("nan"))
        pool[::2] = float("inf")
    return _rehost(k, front_rows, gap_rows, fill), _rehost(v, front_rows, gap_rows, fill)


def neighbours(k, v, n_front, n_behind, value):
    """K and V as row slices ``big[:, n_front:n_front + Nk]`` of [B, n_front + Nk + n_behind, inner] tensors whose other rows hold
    +-``value`` (finite: the rows of the other softmax of an IP-Adapter fallback).  A row read from a neighbour changes the result
    without making it non-finite."""
    out = []
    for t in (k, v):
        B, N, HD = t.shape
        big = torch.empty(B, n_front + N + n_behind, HD, dtype=t.dtype, device=t.device)
        big[:] = value
        big[..., 1::2] = -value
        big[:, n_front:n_front + N] = t
        view = big[:, n_front:n_front + N]
        assert view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 0 and view.stride(1) % 8 == 0
        out.append(view)
    return tuple(out)
