"""Lane-level numpy emulation of k_flash_attn_ip (csrc/attention_kernels.hip): index math only, fp64.

The same expressions as the kernel -- key row -> LDS block, accumulator register -> key index, the mask bounds at Nt and Ni, the
transpose reads of V -- under the MFMA / ds_read_b64_tr_b16 layouts of tools/emulate_flash_attention.py, checked against two plain
softmaxes before any GPU time is spent.  LDS starts poisoned (NaN) and the memory behind the last key row is NaN as well: a
fragment that reads a slot the staging did not write, or a staging read past row Nt + Ni, shows in the result.

    python tools/emulate_flash_attention_ip.py
"""
import numpy as np

from emulate_flash_attention import D, K_LD, QB, V_LD_TR, mfma_32x32x16, tr_read

SK_QBLOCKS = 4


def nkb_of(Nt):
    return 2 if Nt <= 64 else (3 if Nt <= 96 else 5)


def run_workgroup(q, k, v, Nq, Nt, Ni, qgrp, scale, ip_scale):
    """q [Nq,64]; k / v [Nt + Ni + tail,64] with NaN rows from Nt + Ni on -> {row: out[64]} of one workgroup (512 query rows)"""
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
            for r in range(16):
                s[NKB][8 * (r >> 2) + 4 * hi + (r & 3) >= Ni, r] = -np.inf
            mx = s[:NKB].max((0, 2))
            mx = np.maximum(mx, mx[lanes ^ 32])
            e = np.exp2(s[:NKB] * sl - (mx * sl)[None, :, None])
            psum = e.sum((0, 2))
            psum = psum + psum[lanes ^ 32]
            mxi = s[NKB].max(1)
            mxi = np.maximum(mxi, mxi[lanes ^ 32])
            ei = np.exp2(s[NKB] * sl - (mxi * sl)[:, None])
            psi = ei.sum(1)
            psi = psi + psi[lanes ^ 32]
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
            res = o / psum[None, :, None] + ip_scale * (oi / psi[None, :, None])
            for l in range(64):
                if q_row[l] < Nq:
                    dst = out.setdefault(int(q_row[l]), np.full(D, np.nan))
                    for db in range(2):
                        for g in range(4):
                            for e_ in range(4):
                                dst[32 * db + 8 * g + 4 * hi[l] + e_] = res[db][l, 4 * g + e_]
    return out


def softmax_v(q, k, v, scale):
    s = (q @ k.T) * scale
    p = np.exp(s - s.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)) @ v


if __name__ == "__main__":
    rng = np.random.default_rng(0)
    cases = [(100, nt, ni) for nt in (1, 31, 32, 64, 65, 77, 96, 97, 129, 154, 160) for ni in (1, 4, 31, 32)]
    cases += [(513, 77, 4), (1, 154, 16), (640, 1, 1)]
    for Nq, Nt, Ni in cases:
        q = rng.standard_normal((Nq, D))
        k, v = rng.standard_normal((Nt + Ni + 8, D)), rng.standard_normal((Nt + Ni + 8, D))
        k[Nt + Ni:], v[Nt + Ni:] = np.nan, np.nan
        want = softmax_v(q, k[:Nt], v[:Nt], 0.125) + 0.6 * softmax_v(q, k[Nt:Nt + Ni], v[Nt:Nt + Ni], 0.125)
        got = {}
        for qgrp in range((Nq + QB * SK_QBLOCKS - 1) // (QB * SK_QBLOCKS)):
            got.update(run_workgroup(q, k, v, Nq, Nt, Ni, qgrp, 0.125, 0.6))
        err = max(np.abs(got[r] - want[r]).max() for r in got)
        print(f"Nq={Nq} Nt={Nt} Ni={Ni}: rows={len(got)} max|err|={err:.2e}")
        assert len(got) == Nq and err < 1e-12
    print("index math OK")
