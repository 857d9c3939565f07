"""Lane-level numpy emulation of k_flash_attn_ipm (csrc/attention_kernels.hip): index math only, fp64.

k_flash_attn_ipn's replay (tools/emulate_flash_attention_ipn.py) with the one addition of the masked kernel: which lane holds which
query row, and the address of m for it -- ``base + b * m_sb + a * m_sa + q_row`` with ``base`` the offset of the level inside a
row's buffer -- read only for q_row < Nq and a < A.  The mask lives in one flat buffer that is NaN everywhere except at the
elements the rule addresses: behind row Nq - 1 of every adapter, between the levels, in the other batch entries' rows and behind the
last element.  A lane that reads any other word, or the right word for the wrong adapter, shows in the result.

    python tools/emulate_flash_attention_ipm.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from emulate_flash_attention import D, K_LD, QB, V_LD_TR, mfma_32x32x16, tr_read  # noqa: E402
from emulate_flash_attention_ip import SK_QBLOCKS, nkb_of, softmax_v  # noqa: E402
from emulate_flash_attention_ipn import IPN_MAX, WEIGHTS  # noqa: E402

SEGMENTATIONS = [(4,), (32,), (16, 16), (4, 16), (1, 1, 1, 1), (13, 19)]


def run_workgroup(q, k, v, Nq, Nt, segs, qgrp, scale, w, mbuf, m_base, m_sa, reads):
    """one workgroup of batch entry b (``m_base`` = level offset + b * m_sb); ``reads`` collects every address of m it touches"""
    A = len(segs)
    ends = list(np.cumsum(segs)) + [int(sum(segs))] * (IPN_MAX - A)
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
            k_lds[row * K_LD + col: row * K_LD + col + 8] = k[src, col:col + 8] if src < lim else np.zeros(8)
            v_lds[row * V_LD_TR + col: row * V_LD_TR + col + 8] = v[src, col:col + 8] if src < lim else np.zeros(8)
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
            # the kernel's wm[a]: (a < A && q_row < Nq) ? wa[a] * mg[a * m_sa + q_row] : 0
            wm = np.zeros((IPN_MAX, 64))
            for a in range(A):
                for l in range(64):
                    if q_row[l] < Nq:
                        addr = m_base + a * m_sa + int(q_row[l])
                        reads.add(addr)
                        wm[a, l] = wa[a] * mbuf[addr]
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
            si = s[NKB]
            mxa = np.full((IPN_MAX, 64), -np.inf)
            member = np.zeros((IPN_MAX, 64, 16), bool)
            for r in range(16):
                j = 8 * (r >> 2) + 4 * hi + (r & 3)
                seg = sum((j >= ends[a]).astype(int) for a in range(IPN_MAX))
                si[seg == IPN_MAX, r] = -np.inf
                for a in range(A):
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
                ca = [wm[a] * (1.0 / psa[a]) if a < A else np.zeros(64) for a in range(IPN_MAX)]
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


def reference(q, k, v, Nt, segs, scale, w, m):
    """m [A, Nq]"""
    want = softmax_v(q, k[:Nt], v[:Nt], scale)
    off = Nt
    for a, n in enumerate(segs):
        want = want + (w[a] * m[a])[:, None] * softmax_v(q, k[off:off + n], v[off:off + n], scale)
        off += n
    return want


def mask_buffer(rng, B, A, Nq, level_off, level_pad, m_sb_zero):
    """-> (flat NaN-poisoned buffer, m_sb, m_sa, masks [B or 1, A, Nq]): rows of [A, S] with the level at ``level_off`` inside S =
    level_off + Nq + level_pad, valid words only where (b, a, i < Nq) points; with ``m_sb_zero`` one row serves every b"""
    S_ = level_off + Nq + level_pad
    nb = 1 if m_sb_zero else B
    buf = np.full(nb * A * S_ + 4, np.nan)
    m = rng.random((nb, A, Nq))
    m[:, :, 0] = 0.0                                   # planted exact 0 and exact 1 rows
    m[:, :, Nq - 1] = 1.0
    for b in range(nb):
        for a in range(A):
            at = (b * A + a) * S_ + level_off
            buf[at:at + Nq] = m[b, a]
    return buf, (0 if m_sb_zero else A * S_), S_, m


def check_case(Nq, Nt, segs, seed=0, w=WEIGHTS, B=2, level_off=0, level_pad=3, m_sb_zero=False):
    """-> max |emulation - reference| over the rows of every batch entry; asserts the set of mask words read is exactly the valid one"""
    rng = np.random.default_rng(seed)
    A, n = len(segs), Nt + sum(segs)
    buf, m_sb, m_sa, m = mask_buffer(rng, B, A, Nq, level_off, level_pad, m_sb_zero)
    worst = 0.0
    for b in range(B):
        q = rng.standard_normal((Nq, D))
        k, v = rng.standard_normal((n + 8, D)), rng.standard_normal((n + 8, D))
        k[n:], v[n:] = np.nan, np.nan
        mb = m[0 if m_sb_zero else b]
        want = reference(q, k, v, Nt, segs, 0.125, w, mb)
        got, reads = {}, set()
        for qgrp in range((Nq + QB * SK_QBLOCKS - 1) // (QB * SK_QBLOCKS)):
            got.update(run_workgroup(q, k, v, Nq, Nt, segs, qgrp, 0.125, w, buf, level_off + b * m_sb, m_sa, reads))
        assert len(got) == Nq
        valid = {level_off + b * m_sb + a * m_sa + i for a in range(A) for i in range(Nq)}
        assert reads == valid, (sorted(reads - valid)[:4], sorted(valid - reads)[:4])
        worst = max(worst, max(np.abs(got[r] - want[r]).max() for r in got))
    return worst


CASES = [(33, 77, segs, dict()) for segs in SEGMENTATIONS]
CASES += [(100, 97, (4, 16), dict(level_off=64, level_pad=0)), (1, 160, (16, 16), dict(level_off=7)),
          (130, 1, (1, 1, 1, 1), dict(m_sb_zero=True)), (513, 77, (4,), dict(B=1, level_off=12))]


if __name__ == "__main__":
    for Nq, Nt, segs, kw in CASES:
        err = check_case(Nq, Nt, segs, **kw)
        print(f"Nq={Nq} Nt={Nt} segs={segs} {kw}: max|err|={err:.2e}")
        assert err < 1e-12
    print("index math OK")
