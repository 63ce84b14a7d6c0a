"""Restatements for the class-code fine-tuning step (csrc/finetune.hip, sylph_amd/finetune.py).

  fcos_targets_ref   FCOSOutputs.compute_targets_for_locations + get_sample_region (fcos_outputs.py:193-349), labels only, in float32 numpy,
                     comparison by comparison; pinned to the reference itself by tests/golden/g12_fcos_targets.npz
  focal              fvcore's sigmoid_focal_loss and its hand-written derivative, float64
  cls_grad_ref       loss, dW, db of one call in float64 on the operand values the kernel feeds its MFMAs (x normalised to bf16, codes
                     rounded to bf16, g as a bf16 hi + lo pair in dW), with the float64 sums of absolute terms that scale the error bound
"""
import numpy as np
import torch

from oracle import bf16 as OB16

INF = 100000000.0


def levels(hw, n=5):
    out, (h, w) = [], (hw[0] // 8, hw[1] // 8)
    for _ in range(n):
        out.append((h, w))
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return out


def fcos_targets_ref(boxes, classes, image_index, n_images, level_shapes, strides=(8, 16, 32, 64, 128), soi=(64, 128, 256, 512),
                     center_sample=True, radius=1.5):
    """-> int32 labels in the tower output's row order: [image][level][y][x], -1 for background; every location of the padded map"""
    f = np.float32
    boxes = np.asarray(boxes, f).reshape(-1, 4)
    classes = np.asarray(classes).reshape(-1)
    image_index = np.asarray(image_index).reshape(-1)
    lo = [f(-1)] + [f(s) for s in soi]
    hi = [f(s) for s in soi] + [f(INF)]
    out = []
    for b in range(n_images):
        bx, cl = boxes[image_index == b], classes[image_index == b]
        for l, (h, w) in enumerate(level_shapes):
            s = strides[l]
            ys, xs = np.meshgrid(np.arange(h, dtype=np.int64) * s + s // 2, np.arange(w, dtype=np.int64) * s + s // 2, indexing="ij")
            x, y = xs.reshape(-1, 1).astype(f), ys.reshape(-1, 1).astype(f)
            lab = np.full(h * w, -1, np.int32)
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
                k = area.argmin(1)  # the first of equal minima
                lab = np.where(area[np.arange(h * w), k] == f(INF), -1, cl[k]).astype(np.int32)
            out.append(lab)
    return np.concatenate(out)


def focal(z, t, alpha, gamma):
    """fvcore.nn.sigmoid_focal_loss (reduction none) and d loss / d z, elementwise, in the dtype of z.  With u = (2 t - 1) z and
    p_t = sigmoid(u): ce = -log p_t, loss = a_t (1 - p_t)^gamma ce, g = a_t (2 t - 1) (1 - p_t)^gamma (-gamma p_t ce - (1 - p_t))."""
    t = t.to(z.dtype)
    u = (2 * t - 1) * z
    e = torch.exp(-u.abs())
    inv = 1 / (1 + e)
    pt = torch.where(u >= 0, inv, e * inv)
    q = torch.where(u >= 0, e * inv, inv)
    ce = torch.clamp(-u, min=0) + torch.log1p(e)
    at = alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else torch.ones_like(z)
    am = at * q ** gamma
    return am * ce, am * (2 * t - 1) * (-gamma * pt * ce - q)


def focal_fvcore(z, t, alpha, gamma):
    """the formula as fvcore writes it (sigmoid_focal_loss, reduction none): the autograd yardstick of `focal`"""
    import torch.nn.functional as F
    t = t.to(z.dtype)
    p = torch.sigmoid(z)
    ce = F.binary_cross_entropy_with_logits(z, t, reduction="none")
    p_t = p * t + (1 - p) * (1 - t)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss


def rows_of(levels_nchw):
    """per-level (B, C, h, w) maps -> (B * rows, C) in the tower output's row order"""
    B = levels_nchw[0].shape[0]
    return torch.cat([torch.cat([lv[i].flatten(1).t() for lv in levels_nchw]) for i in range(B)])


def cls_grad_ref(xn, labels, w, b, alpha, gamma, class_offset=0):
    """xn: (rows, 256) the normalised bf16 operand values; labels: (rows,) int; w: (N, 256) fp32; b: (N,) or None.
    -> dict of float64 tensors: loss, gw (N, 256), gb (N,) and the sums of absolute terms A_loss, A_gw, A_gb."""
    x = xn.double()
    wq = OB16.r(w.float()).double()
    N = w.shape[0]
    z = x @ wq.t() + (b.double()[None] if b is not None else 0.0)
    t = labels.reshape(-1, 1).long() == (class_offset + torch.arange(N))[None]
    loss, g = focal(z, t, alpha, gamma)
    g32 = g.float()
    hi = OB16.r(g32)
    lo = OB16.r(g32 - hi)
    gq = hi.double() + lo.double()
    return {"loss": loss.sum(), "gw": gq.t() @ x, "gb": g.sum(0),
            "A_loss": loss.abs().sum(), "A_gw": gq.abs().t() @ x.abs(), "A_gb": g.abs().sum(0)}


def sgd_ref(w, grad, buf, lr, momentum, weight_decay):
    """one torch.optim.SGD step (dampening 0, no nesterov) written out: -> (w, buf)"""
    d = grad + weight_decay * w
    buf = d.clone() if buf is None else momentum * buf + d
    return w - lr * buf, buf


# ---- the loop's synthetic task: four records of two 128 x 160 images, three boxes per image, five classes -----------------------------
LOOP_HW, LOOP_RECORDS, LOOP_CLASSES = (128, 160), 4, 5


def pyramid(B, hw, seed):
    """B distinct images of random bf16-representable features (CPU generator: the same numbers on every machine)"""
    g = torch.Generator().manual_seed(seed)
    return [OB16.r(torch.randn(B, 256, h, w, generator=g)) for h, w in levels(hw)]


def random_boxes(n_images, per_image, hw, n_classes, seed, lo=24.0, hi=100.0):
    """-> annotations dict: boxes (n, 4) float32 inside the padded frame, classes (n,), image_index (n,) sorted"""
    g = torch.Generator().manual_seed(seed)
    n = n_images * per_image
    bw, bh = lo + torch.rand(n, generator=g) * (hi - lo), lo + torch.rand(n, generator=g) * (hi - lo)
    x0, y0 = torch.rand(n, generator=g) * (hw[1] - bw), torch.rand(n, generator=g) * (hw[0] - bh)
    return {"boxes": torch.stack([x0, y0, x0 + bw, y0 + bh], 1), "classes": torch.randint(0, n_classes, (n,), generator=g),
            "image_index": torch.arange(n_images).repeat_interleave(per_image)}


def loop_task():
    """-> [(pyramid, annotations)] of the loop test, one per record"""
    return [(pyramid(2, LOOP_HW, 30 + r), random_boxes(2, 3, LOOP_HW, LOOP_CLASSES, 40 + r)) for r in range(LOOP_RECORDS)]


def loop_ref(xns, labels, n_classes, iters, lr, momentum=0.9, weight_decay=1e-4, alpha=0.25, gamma=2.0, prior=0.01):
    """finetune_class_codes restated in float64 on every record per step, from zero codes with the prior bias -> the loss of every step"""
    import math
    w = torch.zeros(n_classes, 256, dtype=torch.float64)
    b = torch.full((n_classes,), -math.log((1 - prior) / prior), dtype=torch.float64)
    npos = max(sum(int((l >= 0).sum()) for l in labels), 1)
    bw = bb = None
    losses = []
    for _ in range(iters):
        out = [cls_grad_ref(x, l, w.float(), b.float(), alpha, gamma) for x, l in zip(xns, labels)]
        losses.append(float(sum(o["loss"] for o in out)) / npos)
        w, bw = sgd_ref(w, sum(o["gw"] for o in out) / npos, bw, lr, momentum, weight_decay)
        b, bb = sgd_ref(b, sum(o["gb"] for o in out) / npos, bb, lr, momentum, weight_decay)
    return losses
