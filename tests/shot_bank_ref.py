"""Float32 numpy restatement of the shot bank's two steps (csrc/shot_bank.hip), for both generators.

pool_rows restates shot_pool_kernel and combine_rows shot_combine_kernel, i.e. together the loops of codegen_tail_kernel
(csrc/codegen.hip): the same operations in the same order with np.float32 at every step -- the sequential sums over positions, the
3 x 3 bins [0,3) [2,5) [4,7), the 64-lane xor tree of the bias and scale heads, the strided softmax (lane l owns shots l, l + 64, ...),
code += w[s] * v in list order.  mean_rows restates mean_tokens_kernel on gathered rows.  Additions, multiplications, divisions and
square roots are IEEE operations and reproduce the device bit for bit; np.exp is another libm than the device's expf, so the softmax
weights are reproduced to an ulp, not to the bit."""
import numpy as np

F = np.float32


def xor_tree(v):
    """for (o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o) over 64 lanes -> the value every lane ends with"""
    t = np.asarray(v, dtype=F).copy()
    assert t.shape == (64,)
    lanes = np.arange(64)
    o = 32
    while o > 0:
        t = (t + t[lanes ^ o]).astype(F)
        o >>= 1
    assert np.all(t == t[0]) or np.any(np.isnan(t))
    return t[0]


def seq_sum(x, axis=0):
    """sum = 0; for p: sum += x[p] (vectorised over the other axes)"""
    x = np.moveaxis(np.asarray(x, dtype=F), axis, 0)
    s = np.zeros(x.shape[1:], dtype=F)
    for p in range(x.shape[0]):
        s = (s + x[p]).astype(F)
    return s


def row_floats(k=1):
    return 256 * k * k + 4


def pool_rows(conv, aux=None, ib=-1, iw=-1, is_=-1, k=1, bias_l2_norm=False):
    """conv (R, 256, 7, 7) fp32, aux (R, naux, 7, 7) fp32 with the bias / shot-weight / class-scale heads at channels ib / iw / is_
    (-1: absent) -> rows (R, 256 k^2 + 4)"""
    conv = np.asarray(conv, dtype=F)
    R, C = conv.shape[:2]
    npos = F(49)
    rows = np.zeros((R, C * k * k + 4), dtype=F)
    if k == 3:
        out = np.zeros((R, C, 3, 3), dtype=F)
        for ky in range(3):
            for kx in range(3):
                y0, x0 = (ky * 7) // 3, (kx * 7) // 3
                s = np.zeros((R, C), dtype=F)
                for dy in range(3):
                    for dx in range(3):
                        s = (s + conv[:, :, y0 + dy, x0 + dx]).astype(F)
                out[:, :, ky, kx] = s / F(9)
        rows[:, :C * 9] = out.reshape(R, C * 9)
    else:
        rows[:, :C] = seq_sum(conv.reshape(R, C, 49), axis=2) / npos
    n = C * k * k
    for r in range(R):
        if ib >= 0:
            v = np.zeros(64, dtype=F)
            v[:49] = aux[r, ib].reshape(49)
            nrm = F(1)
            if bias_l2_norm:
                nrm = np.maximum(np.sqrt(xor_tree((v * v).astype(F))), F(1e-12)).astype(F)
            rows[r, n] = xor_tree((v / nrm).astype(F)) / npos
        if iw >= 0:
            rows[r, n + 1] = seq_sum(np.asarray(aux[r, iw], dtype=F).reshape(49)) / npos
        if is_ >= 0:
            v = np.zeros(64, dtype=F)
            v[:49] = aux[r, is_].reshape(49)
            rows[r, n + 2] = xor_tree(v) / npos
    return rows


def shot_weights(logits, softmax):
    """the S weights of one segment: 1 / S, or the strided softmax of its logits"""
    S = len(logits)
    if not softmax:
        return np.full(S, F(1) / F(S), dtype=F)
    lg = np.asarray(logits, dtype=F)
    mx = F(-np.inf)
    for i in range(S):
        mx = np.maximum(mx, lg[i])
    e = np.exp((lg - mx).astype(F)).astype(F)
    den = np.zeros(64, dtype=F)
    for lane in range(64):
        for i in range(lane, S, 64):
            den[lane] = den[lane] + e[i]
    return (e / xor_tree(den)).astype(F)


def combine_rows(rows, idx, seg_len, k=1, softmax=False):
    """-> (codes (n_seg, 256 k^2 + 1), cls_weight_norm (n_seg,)) of the segments of idx over rows (., 256 k^2 + 4)"""
    rows = np.asarray(rows, dtype=F)
    n = 256 * k * k
    codes = np.zeros((len(seg_len), n + 1), dtype=F)
    wn = np.zeros(len(seg_len), dtype=F)
    i0 = 0
    for j, S in enumerate(seg_len):
        g = rows[np.asarray(idx[i0:i0 + S])]
        w = shot_weights(g[:, n + 1], softmax)
        code, bias, scale = np.zeros(n, dtype=F), F(0), F(0)
        for s in range(S):
            code = (code + (w[s] * g[s, :n]).astype(F)).astype(F)
            bias = F(bias + F(w[s] * g[s, n]))
            scale = F(scale + F(w[s] * g[s, n + 2]))
        codes[j, :n], codes[j, n], wn[j] = code, bias, scale
        i0 += S
    return codes, wn


def mean_rows(rows, idx, seg_len):
    """mean_tokens_kernel on gathered ROIEncoder rows (., 260): additions in list order, one division -> (n_seg, 256)"""
    rows = np.asarray(rows, dtype=F)
    out = np.zeros((len(seg_len), 256), dtype=F)
    i0 = 0
    for j, S in enumerate(seg_len):
        out[j] = seq_sum(rows[np.asarray(idx[i0:i0 + S]), :256], axis=0) / F(S)
        i0 += S
    return out
