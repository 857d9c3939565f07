"""Lane-level numpy emulation of k_flash_attn_ipn (csrc/attention_kernels.hip): index math only, fp64.

The same expressions as the kernel -- key row -> LDS row, accumulator register -> key index -> segment, the mask bounds at Nt and
at the end of the last segment, the per-segment maxima and sums, the pre-normalised and weighted probabilities, the transpose
reads of V -- under the MFMA / ds_read_b64_tr_b16 layouts of tools/emulate_flash_attention.py, checked against A + 1 plain
softmaxes before any GPU time is spent.  LDS starts poisoned (NaN) and the memory behind the last key row is NaN as well: a
fragment that reads a slot the staging did not write, or a staging read past the last image row, shows in the result.

    python tools/emulate_flash_attention_ipn.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from emulate_flash_attention import D, K_LD, QB, V_LD_TR, mfma_32x32x16, tr_read  # noqa: E402
from emulate_flash_attention_ip import SK_QBLOCKS, nkb_of, softmax_v  # noqa: E402

IPN_MAX = 4
# the segmentations of the GPU tests: boundaries inside a lane's group of four keys, between the two half-waves' groups, on 8-key groups
SEGMENTATIONS = [(1, 1), (4, 4), (16, 16), (3, 5), (13, 19), (4, 16, 4), (1, 30, 1), (8, 8, 8, 8), (31, 1)]
WEIGHTS = (0.6, 1.0, -0.5, 0.3)


def segment_of_register(r, hi, ends):
    """accumulator register r of half-wave hi -> (key index inside the image block, segment or None): the kernel's predicate"""
    j = 8 * (r >> 2) + 4 * hi + (r & 3)
    seg = sum(1 for a in range(IPN_MAX) if j >= ends[a])      # the number of segment ends at or below the key index
    return j, (seg if seg < IPN_MAX else None)


def run_workgroup(q, k, v, Nq, Nt, segs, qgrp, scale, w):
    """q [Nq,64]; k / v [Nt + sum(segs) + tail,64] with NaN rows behind the last image row -> {row: out[64]} of one workgroup"""
    A = len(segs)
    ends = list(np.cumsum(segs)) + [int(sum(segs))] * (IPN_MAX - A)      # the entry point's ParamsIpn.end
    Ni = ends[IPN_MAX - 1]
    wa = [w[a] if a < A else 0.0 for a in range(IPN_MAX)]
    NKB = nkb_of(Nt)
    rows = 32 * (NKB + 1)
    k_lds, v_lds = np.full(rows * K_LD, np.nan), np.full(rows * V_LD_TR, np.nan)
    for tid in range(256):
        for idx in range(tid, rows * 8, 256):
            row, col = idx >> 3, (idx & 7) * 8
            img = row >= 32 * NKB
            j = row - 32 * NKB
            src = Nt + j if img else row
            lim = Nt + Ni if img else Nt
            kr = k[src, col:col + 8] if src < lim else np.zeros(8)
            vr = v[src, col:col + 8] if src < lim else np.zeros(8)
            k_lds[row * K_LD + col: row * K_LD + col + 8] = kr
            v_lds[row * V_LD_TR + col: row * V_LD_TR + col + 8] = vr
    out = {}
    sl = scale * np.log2(np.e)
    lanes = np.arange(64)
    ln, hi = lanes & 31, lanes >> 5
    for wave in range(4):
        for qb in range(SK_QBLOCKS):
            base = (qgrp * SK_QBLOCKS + qb) * QB + wave * 32
            if base >= Nq:
                break
            q_row = base + ln
            qf = np.zeros((4, 64, 8))
            for ks in range(4):
                for l in range(64):
                    if q_row[l] < Nq:
                        qf[ks, l] = q[q_row[l], 16 * ks + 8 * hi[l]: 16 * ks + 8 * hi[l] + 8]
            s = np.zeros((NKB + 1, 64, 16))
            for ks in range(4):
                for kb in range(NKB + 1):
                    kf = np.zeros((64, 8))
                    for l in range(64):
                        a0 = (32 * kb + ln[l]) * K_LD + 16 * ks + 8 * hi[l]
                        kf[l] = k_lds[a0:a0 + 8]
                    s[kb] = mfma_32x32x16(kf, qf[ks], s[kb])
            for kb in range(NKB):
                for r in range(16):
                    s[kb][32 * kb + 8 * (r >> 2) + 4 * hi + (r & 3) >= Nt, r] = -np.inf
            mx = s[:NKB].max((0, 2))
            mx = np.maximum(mx, mx[lanes ^ 32])
            e = np.exp2(s[:NKB] * sl - (mx * sl)[None, :, None])
            psum = e.sum((0, 2))
            psum = psum + psum[lanes ^ 32]
            # image block: a maximum and a sum per segment
            si = s[NKB]
            mxa = np.full((IPN_MAX, 64), -np.inf)
            member = np.zeros((IPN_MAX, 64, 16), bool)
            for r in range(16):
                j = 8 * (r >> 2) + 4 * hi + (r & 3)
                seg = sum((j >= ends[a]).astype(int) for a in range(IPN_MAX))
                si[seg == IPN_MAX, r] = -np.inf
                for a in range(A):                       # segments from A on are empty: skipped
                    member[a, :, r] = seg == a
                    mxa[a] = np.maximum(mxa[a], np.where(member[a, :, r], si[:, r], -np.inf))
            mxa = np.maximum(mxa, mxa[:, lanes ^ 32])
            mba = mxa * sl
            psa = np.zeros((IPN_MAX, 64))
            ei = np.zeros((64, 16))
            for r in range(16):
                ref = np.zeros(64)
                for a in range(IPN_MAX):
                    ref = np.where(member[a, :, r], mba[a], ref)
                ei[:, r] = np.exp2(si[:, r] * sl - ref)
                for a in range(IPN_MAX):
                    psa[a] += np.where(member[a, :, r], ei[:, r], 0.0)
            psa = psa + psa[:, lanes ^ 32]
            with np.errstate(divide="ignore"):
                ca = [wa[a] * (1.0 / psa[a]) if a < A else np.zeros(64) for a in range(IPN_MAX)]
            for r in range(16):
                c = np.zeros(64)
                for a in range(IPN_MAX):
                    c = np.where(member[a, :, r], ca[a], c)
                ei[:, r] *= c
            o, oi = np.zeros((2, 64, 16)), np.zeros((2, 64, 16))
            for st in range(2 * NKB + 2):
                text = st < 2 * NKB
                src = e[st >> 1] if text else ei
                pf = src[:, 8 * (st & 1): 8 * (st & 1) + 8]
                for db in range(2):
                    row = 16 * st + 4 * hi + ((lanes & 15) >> 2)
                    col = 32 * db + 16 * ((lanes >> 4) & 1) + 4 * (lanes & 3)
                    vf = np.concatenate([tr_read(v_lds, row * V_LD_TR + col), tr_read(v_lds, (row + 8) * V_LD_TR + col)], 1)
                    if text:
                        o[db] = mfma_32x32x16(vf, pf, o[db])
                    else:
                        oi[db] = mfma_32x32x16(vf, pf, oi[db])
            res = o / psum[None, :, None] + oi
            for l in range(64):
                if q_row[l] < Nq:
                    dst = out.setdefault(int(q_row[l]), np.full(D, np.nan))
                    for db in range(2):
                        for g in range(4):
                            for e_ in range(4):
                                dst[32 * db + 8 * g + 4 * hi[l] + e_] = res[db][l, 4 * g + e_]
    return out


def reference(q, k, v, Nt, segs, scale, w):
    want = softmax_v(q, k[:Nt], v[:Nt], scale)
    off = Nt
    for a, n in enumerate(segs):
        want = want + w[a] * softmax_v(q, k[off:off + n], v[off:off + n], scale)
        off += n
    return want


def check_registers(segs):
    """every key of every segment is held by exactly one (half-wave, register) and lands in its own segment; keys past the end in none"""
    ends = list(np.cumsum(segs)) + [int(sum(segs))] * (IPN_MAX - len(segs))
    seen = {}
    for hi in range(2):
        for r in range(16):
            j, a = segment_of_register(r, hi, ends)
            assert j not in seen
            seen[j] = a
    assert sorted(seen) == list(range(32))
    want = [a for a, n in enumerate(segs) for _ in range(n)] + [None] * (32 - sum(segs))
    assert [seen[j] for j in range(32)] == want, (segs, seen)


def check_case(Nq, Nt, segs, seed=0, w=WEIGHTS):
    """-> max |emulation - reference| over all rows (and asserts every row was written)"""
    rng = np.random.default_rng(seed)
    n = Nt + sum(segs)
    q = rng.standard_normal((Nq, D))
    k, v = rng.standard_normal((n + 8, D)), rng.standard_normal((n + 8, D))
    k[n:], v[n:] = np.nan, np.nan
    want = reference(q, k, v, Nt, segs, 0.125, w)
    got = {}
    for qgrp in range((Nq + QB * SK_QBLOCKS - 1) // (QB * SK_QBLOCKS)):
        got.update(run_workgroup(q, k, v, Nq, Nt, segs, qgrp, 0.125, w))
    assert len(got) == Nq
    return max(np.abs(got[r] - want[r]).max() for r in got)


if __name__ == "__main__":
    for segs in SEGMENTATIONS:
        check_registers(segs)
    cases = [(33, nt, segs) for nt in (1, 77, 96, 97, 154, 160) for segs in SEGMENTATIONS]
    cases += [(513, 77, (4, 16)), (1, 154, (16, 16)), (100, 77, (7,))]
    for Nq, Nt, segs in cases:
        err = check_case(Nq, Nt, segs)
        print(f"Nq={Nq} Nt={Nt} segs={segs}: max|err|={err:.2e}")
        assert err < 1e-12
    print("index math OK")
