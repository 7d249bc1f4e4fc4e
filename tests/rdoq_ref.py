"""NumPy restatement of rate-distortion optimised quantisation against the .nic priors (DESIGN.md
§25; include/nic.h nic_rdoq).  Priors, contexts and files are rans2_ref's and rans3_ref's.  Nothing
here touches the library.

Per latent byte with code r (u8) and pre-quant value f (fp32 in [0, 1]):
  v = f * 255 and e = v - r in fp32; alt = r + 1 if e > 0, r - 1 if e < 0, r if e == 0 (held inside
  0..255); candidate 0 is r, candidate 1 is alt
  D(q) = int(rint((v - q) * (v - q) * 65536)) << 16, every operation rounded to fp32
  rate(q | row F) = lam_fix * COST16[F[q]], lam_fix = round(lam * 65536)
Static prior: the candidate with the smaller D + rate under the channel's row, a tie to r.
Context prior: a two-state Viterbi pass over every (segment, channel) chain; the row of pixel p is
context 0 at the segment's first pixel, else min(2, |q[p-1] - anchor|) of the code kept for p - 1;
ties go to state 0, forward and at the end.
"""
import numpy as np

from tests import rans2_ref as R2
from tests import rans3_ref as R3

CH = R2.CH
COST16 = np.array(R2.COST16, np.int64)
LAM_MAX = 16.0
SEG_MAX = 64


def lam_fix_of(lam):
    if not 0.0 <= lam <= LAM_MAX:
        raise ValueError(f"lam {lam} not in [0, {LAM_MAX}]")
    return int(round(lam * 65536))


def candidates(z, f):
    """codes (..., 96) u8 and pre-quant values (..., 96) fp32 -> (cand (..., 96, 2) int64, the codes r
    and alt; D (..., 96, 2) int64, their distortions)."""
    r = np.asarray(z).astype(np.int64)
    v = np.asarray(f, np.float32) * np.float32(255.0)
    e = v - r.astype(np.float32)
    alt = np.clip(np.where(e > 0, r + 1, np.where(e < 0, r - 1, r)), 0, 255)
    d = np.stack([e, v - alt.astype(np.float32)], -1)
    assert d.dtype == np.float32
    D = np.rint(d * d * np.float32(65536.0)).astype(np.int64) << 16
    return np.stack([r, alt], -1), D


def rdoq_static(z, f, prior, lam_fix):
    """(..., 96) u8 codes -> the codes chosen under the static prior (96 x 256 freqs)."""
    cand, D = candidates(z, f)
    cost = COST16[np.asarray(prior, np.int64)]  # (96, 256)
    c = np.arange(CH).reshape((1,) * (cand.ndim - 2) + (CH, 1))
    J = D + lam_fix * cost[c, cand]
    return np.where(J[..., 1] < J[..., 0], cand[..., 1], cand[..., 0]).astype(np.uint8)


def chain_cost(choice, cand, D, cost_rows, anchor, lam_fix):
    """The priced cost of one chain: choice (L,) in {0, 1}, cand / D (L, 2), cost_rows (3, 256) =
    COST16 of the channel's three rows."""
    total, k = 0, 0
    for p, b in enumerate(choice):
        q = int(cand[p][b])
        total += int(D[p][b]) + lam_fix * int(cost_rows[k][q])
        k = min(2, abs(q - anchor))
    return total


def trellis_chain(cand, D, cost_rows, anchor, lam_fix):
    """One chain, scalar: -> (choice (L,) in {0, 1}, its priced cost)."""
    n = len(cand)
    best = [int(D[0][b]) + lam_fix * int(cost_rows[0][int(cand[0][b])]) for b in (0, 1)]
    back = []
    for p in range(1, n):
        ctx = [min(2, abs(int(cand[p - 1][b]) - anchor)) for b in (0, 1)]
        nxt, bp = [], []
        for b in (0, 1):
            q = int(cand[p][b])
            via = [best[a] + lam_fix * int(cost_rows[ctx[a]][q]) for a in (0, 1)]
            a = 1 if via[1] < via[0] else 0
            bp.append(a)
            nxt.append(int(D[p][b]) + via[a])
        back.append(bp)
        best = nxt
    b = 1 if best[1] < best[0] else 0
    total = best[b]
    choice = [0] * n
    for p in range(n - 1, -1, -1):
        choice[p] = b
        if p:
            b = back[p - 1][b]
    return choice, total


def _rdoq_context_image(z, f, cprior, lam_fix, seg_pixels):
    anchors, freqs = cprior
    A = np.asarray(anchors, np.int64)
    cost = COST16[np.asarray(freqs, np.int64)]  # (96, 3, 256)
    cand, D = candidates(z.reshape(-1, CH), f.reshape(-1, CH))  # (P, 96, 2)
    P, c = cand.shape[0], np.arange(CH)
    out = np.empty((P, CH), np.int64)
    for s0 in range(0, P, seg_pixels):
        n = min(seg_pixels, P - s0)
        bp = np.zeros((n, CH, 2), np.int64)
        best = D[s0] + lam_fix * cost[c[:, None], 0, cand[s0]]
        for p in range(1, n):
            ctx = np.minimum(2, np.abs(cand[s0 + p - 1] - A[:, None]))  # (96, previous state)
            # tot[c, previous state, state]
            tot = best[:, :, None] + lam_fix * cost[c[:, None, None], ctx[:, :, None], cand[s0 + p][:, None, :]]
            bp[p] = np.argmin(tot, 1)  # the first minimum: a tie to state 0
            best = D[s0 + p] + np.min(tot, 1)
        b = np.argmin(best, 1)
        for p in range(n - 1, -1, -1):
            out[s0 + p] = cand[s0 + p][c, b]
            if p:
                b = bp[p][c, b]
    return out.reshape(z.shape).astype(np.uint8)


def rdoq_context(z, f, cprior, lam_fix, seg_pixels=32):
    """(h8, w8, 96) or (N, h8, w8, 96) u8 codes -> the codes chosen under the context prior."""
    if not 1 <= seg_pixels <= SEG_MAX:
        raise ValueError(f"seg_pixels {seg_pixels} not in 1..{SEG_MAX}")
    z, f = np.asarray(z, np.uint8), np.asarray(f, np.float32)
    if z.ndim == 3:
        return _rdoq_context_image(z, f, cprior, lam_fix, seg_pixels)
    return np.stack([_rdoq_context_image(a, b, cprior, lam_fix, seg_pixels) for a, b in zip(z, f)])


def priced_cost_static(zq, f, prior, lam_fix):
    """J of the codes zq (each within 1 of f's code) under the static prior: a Python int."""
    v = np.asarray(f, np.float32) * np.float32(255.0)
    d = v - np.asarray(zq).astype(np.float32)
    D = np.rint(d * d * np.float32(65536.0)).astype(np.int64) << 16
    cost = COST16[np.asarray(prior, np.int64)]
    c = np.arange(CH).reshape((1,) * (np.ndim(zq) - 1) + (CH,))
    return int(D.sum()) + lam_fix * int(cost[c, np.asarray(zq).astype(np.int64)].sum())


def priced_cost_context(zq, f, cprior, lam_fix, seg_pixels=32):
    """J of one image's codes zq (h8, w8, 96) under the context prior: a Python int."""
    anchors, freqs = cprior
    v = np.asarray(f, np.float32).reshape(-1, CH) * np.float32(255.0)
    q = np.asarray(zq).reshape(-1, CH).astype(np.int64)
    d = v - q.astype(np.float32)
    D = np.rint(d * d * np.float32(65536.0)).astype(np.int64) << 16
    ctx = R3.contexts_of(zq, anchors, seg_pixels)
    cost = COST16[np.asarray(freqs, np.int64)]
    return int(D.sum()) + lam_fix * int(cost[np.arange(CH)[None], ctx, q].sum())
