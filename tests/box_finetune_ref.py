"""Restatements for the box-branch fine-tuning step (csrc/box_finetune.hip, sylph_amd/finetune.py: finetune_box_branch).

  box_samples_ref    compute_targets_for_locations + get_sample_region (fcos_outputs.py:193-349) with the regression targets of
                     fcos_outputs.py:185-189, float32 numpy, comparison by comparison: the positives in the tower output's row order;
                     pinned to the reference itself by tests/golden/g13_box_losses.npz
  box_losses         the box losses of fcos_losses (fcos_outputs.py:675-741; iou_loss.py:26-65; compute_ctrness_targets :52-60), written
                     as the reference writes them, in the dtype of its arguments: the autograd yardstick
  box_grad_terms     the same losses with the hand-written derivative d loss / d z per sample and channel, and T, the sum of the
                     absolute values of the derivative's terms that scales the rounding bound (below)
  patches_ref        the host gather of the 3 x 3 x 256 patches from the normalised tower output

The rounding bound of g (stage 2 of tests/test_box_finetune_gpu.py): |g_kernel - g_float64| <= G_ROUNDINGS 2^-24 T at the kernel's own z.
box_loss_one (csrc/box_finetune.hip) evaluates, per side i, g_i = s [s z_i > 0] wgt (-(dai U - A dau) / U^2 - (dau ac - au dac) / ac^2).
Every fp32 operation rounds once (relative 2^-24); min, max, ReLU and the comparisons are exact.  Roundings on the way to a leaf value:
p = s z (1), a side sum such as p0 + p2 (1), a product such as ai = wi hi (1), au = ta + pa - ai (2), U = au + 1 / A = ai + 1 (1): 6.  A
denominator U^2 carries its leaf twice plus the square (13); the numerator dai U - A dau its leaves (6) plus dau, two products and the
difference (4): 10; then the quotient (1), the sum of the two fractions (1), the weight (1), the factor s with the ReLU mask (1), and the
centerness target behind the weight (two quotients, a product, the root: 4).  13 + 10 + 1 + 1 + 1 + 1 + 4 = 31 <= G_ROUNDINGS = 32.
Roundings in front of a subtraction are amplified by the ratio of the sum of absolute values to the result; T therefore evaluates the
formula with every subtraction replaced by the sum of absolute values -- dau -> dpa + dai, au -> ta + pa + ai -- and multiplies the U
terms by kappa^2, kappa = (ta + pa + ai + 1) / U >= 1 (ai <= min(ta, pa), so kappa <= 3), which covers the amplified roundings inside
the squared denominator; ac is a product of sums of non-negative values and needs no such factor.  The two BCE channels are g =
sigmoid(z) - t: exp (<= 2 ulp), 1 + e, the quotient, the target (the centerness target: 4; the IoU target A / U: 6 + 6 kappa + 1) and
the difference stay below the same count with T = sigmoid(z) + kappa t.
"""
import numpy as np
import torch

from oracle import bf16 as OB16

INF = 100000000.0
G_ROUNDINGS = 32
STRIDES = (8, 16, 32, 64, 128)
SOI = (64, 128, 256, 512)


def box_samples_ref(boxes, classes, image_index, n_images, level_shapes, strides=STRIDES, soi=SOI, center_sample=True, radius=1.5):
    """-> (info (n, 4) int32 = (row, level, box index, class), targets (n, 4) float32 = (l, t, r, b) / stride), rows ascending in the tower
    output's order [image][level][y][x]; also the full per-(image, level) tables for the golden: labels and reg targets."""
    f = np.float32
    boxes = np.asarray(boxes, f).reshape(-1, 4)
    classes = np.asarray(classes).reshape(-1)
    image_index = np.asarray(image_index).reshape(-1)
    lo = [f(-1)] + [f(s) for s in soi]
    hi = [f(s) for s in soi] + [f(INF)]
    info, targets, tables = [], [], {}
    row0 = 0
    for b in range(n_images):
        idx = np.nonzero(image_index == b)[0]
        bx = boxes[idx]
        for l, (h, w) in enumerate(level_shapes):
            s = strides[l]
            ys, xs = np.meshgrid(np.arange(h, dtype=np.int64) * s + s // 2, np.arange(w, dtype=np.int64) * s + s // 2, indexing="ij")
            x, y = xs.reshape(-1, 1).astype(f), ys.reshape(-1, 1).astype(f)
            k = np.full(h * w, -1, np.int64)
            reg = np.zeros((h * w, 4), f)
            if len(bx):
                x0, y0, x1, y1 = (bx[None, :, i] for i in range(4))
                ltrb = np.stack([x - x0, y - y0, x1 - x, y1 - y], -1)
                if center_sample:
                    cx, cy = (x0 + x1) * f(0.5), (y0 + y1) * f(0.5)
                    if cx[0, 0] == 0:  # `center_x[..., 0].sum() == 0`: the FIRST box decides for the image
                        inside = np.zeros((h * w, len(bx)), bool)
                    else:
                        st = f(s * radius)
                        xmin, ymin, xmax, ymax = cx - st, cy - st, cx + st, cy + st
                        c0, c1 = np.where(xmin > x0, xmin, x0), np.where(ymin > y0, ymin, y0)
                        c2, c3 = np.where(xmax > x1, x1, xmax), np.where(ymax > y1, y1, ymax)
                        inside = np.stack([x - c0, y - c1, c2 - x, c3 - y], -1).min(-1) > 0
                else:
                    inside = ltrb.min(-1) > 0
                m = ltrb.max(-1)
                cared = (m >= lo[l]) & (m <= hi[l])
                area = np.broadcast_to(((bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1]))[None], inside.shape).astype(f).copy()
                area[~inside] = INF
                area[~cared] = INF
                kk = area.argmin(1)  # the first of equal minima
                reg = (ltrb[np.arange(h * w), kk] / f(s)).astype(f)
                k = np.where(area[np.arange(h * w), kk] == f(INF), -1, idx[kk])
            tables[(b, l)] = (k, reg)
            for i in np.nonzero(k >= 0)[0]:
                info.append((row0 + i, l, k[i], classes[k[i]]))
                targets.append(reg[i])
            row0 += h * w
    return (np.array(info, np.int32).reshape(-1, 4), np.array(targets, np.float32).reshape(-1, 4), tables)


def ctrness_targets(tau):
    """fcos_outputs.py:52-60"""
    lr, tb = tau[:, [0, 2]], tau[:, [1, 3]]
    return torch.sqrt((lr.min(-1)[0] / lr.max(-1)[0]) * (tb.min(-1)[0] / tb.max(-1)[0]))


def compute_ious(pred, target):
    """iou_loss.py:26-65, line by line"""
    pl, pt, pr, pb = pred.unbind(1)
    tl, tt, tr, tb = target.unbind(1)
    target_area = (tl + tr) * (tt + tb)
    pred_area = (pl + pr) * (pt + pb)
    w_int = torch.min(pl, tl) + torch.min(pr, tr)
    h_int = torch.min(pb, tb) + torch.min(pt, tt)
    g_w = torch.max(pl, tl) + torch.max(pr, tr)
    g_h = torch.max(pb, tb) + torch.max(pt, tt)
    ac = g_w * g_h
    area_int = w_int * h_int
    area_union = target_area + pred_area - area_int
    ious = (area_int + 1.0) / (area_union + 1.0)
    gious = ious - (ac - area_union) / ac
    return ious, gious


def _q(quality):
    q = sorted(quality)
    assert q in (["ctrness"], ["iou"], ["ctrness", "iou"]), q
    return q


def box_losses(reg_pred, ctr_pred, iou_pred, tau, quality, iou_mask):
    """fcos_outputs.py:675-741 on one rank, as written there: reg_pred (n, 4) the served regression (after Scale and ReLU), ctr_pred /
    iou_pred (n,) logits (iou_pred None: no such channel).  -> dict of UN-normalised sums loc, ctr, iou, ctr_sum (0-d tensors) -- the
    sum the trained parameters see is `total`: only the losses fcos_losses returns for this BOX_QUALITY."""
    import torch.nn.functional as F
    q = _q(quality)
    ious, gious = compute_ious(reg_pred, tau)
    iou_t = ious.detach().clone()
    if iou_mask:
        iou_t[iou_t < 0.3] = 0
    ctr_t = ctrness_targets(tau)
    ctr = F.binary_cross_entropy_with_logits(ctr_pred, ctr_t, reduction="sum")
    iou = F.binary_cross_entropy_with_logits(iou_pred, iou_t, reduction="sum") if iou_pred is not None else reg_pred.sum() * 0
    loc = ((1 - gious) * ctr_t).sum() if "ctrness" in q else (1 - gious).sum()
    total = loc + (ctr if "ctrness" in q else 0) + (iou if "iou" in q else 0)
    return {"loc": loc, "ctr": ctr, "iou": iou, "ctr_sum": ctr_t.sum(), "total": total}


def normalised(sums, n, quality):
    """(loc, ctr, iou) as fcos_losses returns them on one rank: loc / max(ctr_sum, 1e-6) with "ctrness", else / num_pos_avg = max(n, 1)"""
    npos = max(float(n), 1.0)
    den = max(float(sums["ctr_sum"]), 1e-6) if "ctrness" in _q(quality) else npos
    return float(sums["loc"]) / den, float(sums["ctr"]) / npos, float(sums["iou"]) / npos


def branch_forward(z, scale_of_sample):
    """z (n, Cout) pre-activations -> (reg_pred, ctr_pred, iou_pred or None): relu(scale z[:, :4]), z[:, 4], z[:, 5]"""
    return torch.relu(scale_of_sample[:, None] * z[:, :4]), z[:, 4], (z[:, 5] if z.shape[1] > 5 else None)


def box_grad_terms(z, tau, scale_of_sample, quality, iou_mask):
    """The hand-written derivative, in the dtype of z (float64 in the tests).  -> dict: g (n, Cout) = d total / d z; gscale (n,) =
    d total / d scale per sample; T (n, Cout) the sum of absolute terms of g (see the module docstring); per-sample losses loc, ctr, iou and
    ctr_t; margin (n,): the smallest distance of s z_i from 0 and of relu(s z_i) from tau_i over the four sides (the kinks)."""
    q = _q(quality)
    s = scale_of_sample
    u = s[:, None] * z[:, :4]
    p = torch.relu(u)
    ta = (tau[:, 0] + tau[:, 2]) * (tau[:, 1] + tau[:, 3])
    pw, ph = p[:, 0] + p[:, 2], p[:, 1] + p[:, 3]
    pa = pw * ph
    wi = torch.min(p[:, 0], tau[:, 0]) + torch.min(p[:, 2], tau[:, 2])
    hi = torch.min(p[:, 3], tau[:, 3]) + torch.min(p[:, 1], tau[:, 1])
    gw = torch.max(p[:, 0], tau[:, 0]) + torch.max(p[:, 2], tau[:, 2])
    gh = torch.max(p[:, 3], tau[:, 3]) + torch.max(p[:, 1], tau[:, 1])
    ac, ai = gw * gh, wi * hi
    au = ta + pa - ai
    A, U = ai + 1, au + 1
    iou = A / U
    giou = iou - (ac - au) / ac
    ctr_t = ctrness_targets(tau)
    wgt = ctr_t if "ctrness" in q else torch.ones_like(ctr_t)
    kappa = (ta + pa + ai + 1) / U
    g = torch.zeros_like(z)
    T = torch.zeros_like(z)
    gscale = torch.zeros_like(s)
    for i in range(4):
        horiz = i % 2 == 0
        dpa = ph if horiz else pw
        dai = torch.where(p[:, i] < tau[:, i], hi if horiz else wi, torch.zeros_like(s))
        dac = torch.where(p[:, i] > tau[:, i], gh if horiz else gw, torch.zeros_like(s))
        dau = dpa - dai
        dg = (dai * U - A * dau) / U ** 2 + (dau * ac - au * dac) / ac ** 2
        on = (u[:, i] > 0).to(z.dtype)
        gp = -wgt * dg * on
        g[:, i] = gp * s
        gscale = gscale + gp * z[:, i]
        aau, adau = ta + pa + ai, dpa + dai
        T[:, i] = s.abs() * on * wgt * (kappa ** 2 * (dai * U + A * adau) / U ** 2 + (adau * ac + aau * dac) / ac ** 2)
    sig = torch.sigmoid(z[:, 4])
    bce = lambda x, t: torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    out = {"loc": wgt * (1 - giou), "ctr": bce(z[:, 4], ctr_t), "ctr_t": ctr_t}
    if "ctrness" in q:
        g[:, 4] = sig - ctr_t
        T[:, 4] = sig + ctr_t
    if z.shape[1] > 5:
        iou_t = torch.where(iou < 0.3, torch.zeros_like(iou), iou) if iou_mask else iou
        out["iou"] = bce(z[:, 5], iou_t)
        if "iou" in q:
            g[:, 5] = torch.sigmoid(z[:, 5]) - iou_t
            T[:, 5] = torch.sigmoid(z[:, 5]) + kappa * iou_t
    else:
        out["iou"] = torch.zeros_like(s)
    margin = torch.minimum(u.abs(), (p - tau).abs()).min(1)[0]
    out.update({"g": g, "gscale": gscale, "T": T, "margin": margin, "iou_value": iou})
    return out


def pack_w(w):
    """(Cout, 256, 3, 3) -> (Cout, 2304) in the patches' k order (ky, kx, c), rounded to bf16 as the kernel rounds it"""
    return OB16.r(w.float()).permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def patches_ref(xn_levels, info, level_shapes):
    """xn_levels: per level (B, 256, h, w) normalised tower output (bf16 values); info (n, 4) -> (n, 3, 3, 256) with zero taps outside"""
    rows_per_image = sum(h * w for h, w in level_shapes)
    off = np.cumsum([0] + [h * w for h, w in level_shapes])
    out = torch.zeros(len(info), 3, 3, 256)
    for p, (row, l, _, _) in enumerate(np.asarray(info)):
        b, i = divmod(int(row), rows_per_image)
        i -= off[l]
        h, w = level_shapes[l]
        y, x = divmod(i, w)
        for ky in range(3):
            for kx in range(3):
                yy, xx = y + ky - 1, x + kx - 1
                if 0 <= yy < h and 0 <= xx < w:
                    out[p, ky, kx] = xn_levels[l][b, :, yy, xx]
    return out
