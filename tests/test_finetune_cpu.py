"""Class-code fine-tuning, host side: the restatements of tests/finetune_ref.py against the reference's golden targets and against torch
autograd, and the optimiser wrapper of sylph_amd/finetune.py against torch.optim.SGD written out.  No GPU."""
import os

import numpy as np
import pytest
import torch

import finetune_ref as FR

CASES = ("a_on", "a_off", "b_on", "c_on", "d_on")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_fcos_targets.npz"))


def golden_labels(g, case):
    """the reference's per-level (B, h w) labels -> the tower output's row order, background -1"""
    per_level = [g[f"{case}_labels{l}"] for l in range(5)]
    rows = np.concatenate([np.concatenate([lv[i] for lv in per_level]) for i in range(2)])
    return np.where(rows == int(g["back_ground_id"]), -1, rows).astype(np.int32)


@pytest.mark.parametrize("case", CASES)
def test_targets_restatement_equals_reference(golden, case):
    g = golden
    hw = tuple(int(v) for v in g["padded_hw"])
    want = golden_labels(g, case)
    got = FR.fcos_targets_ref(g[f"{case}_boxes"], g[f"{case}_classes"], g[f"{case}_image"], 2, FR.levels(hw),
                              center_sample=bool(g[f"{case}_center_sample"]), radius=float(g["pos_radius"]))
    assert got.shape == want.shape == (640 + 160 + 40 + 12 + 4,)  # both images
    assert np.array_equal(got, want), f"{case}: {int((got != want).sum())} labels differ from the reference"


def test_golden_holds_the_required_cases(golden):
    g = golden
    a = golden_labels(g, "a_on").reshape(2, -1)
    assert (a[1] == -1).all() and (a[0] >= 0).any(), "an image with no box"
    assert set(np.unique(a[0])) >= {0, 1, 2, 3}, "whole-image box, sub-cell box and both equal-area boxes claim locations"
    bx = g["a_on_boxes"]
    assert (bx[2, 2] - bx[2, 0]) * (bx[2, 3] - bx[2, 1]) == (bx[3, 2] - bx[3, 0]) * (bx[3, 3] - bx[3, 1])
    assert bx[1, 2] - bx[1, 0] < 8 and bx[1, 3] - bx[1, 1] < 8
    assert not np.array_equal(a, golden_labels(g, "a_off").reshape(2, -1)), "centre sampling changes the labels"
    # b: a location whose largest regression target is exactly 64 resp. 128 is positive on BOTH levels that share the boundary
    lv = FR.levels((128, 160))
    off = np.cumsum([0] + [h * w for h, w in lv])
    b, d = golden_labels(g, "b_on").reshape(2, -1), golden_labels(g, "d_on").reshape(2, -1)

    def at(lab, img, level, x, y):
        s = 8 << level
        return lab[img, off[level] + (y - s // 2) // s * lv[level][1] + (x - s // 2) // s]
    assert at(b, 0, 0, 60, 68) == 0 and at(b, 1, 1, 72, 72) == 1, "largest target exactly 64: <= on P3, >= on P4"
    assert at(d, 0, 1, 136, 72) == 3 and at(d, 1, 2, 144, 48) == 2, "largest target exactly 128: <= on P4, >= on P5"
    c = golden_labels(g, "c_on").reshape(2, -1)
    assert (c[1] == -1).all() and (c[0] >= 0).any(), "first box with centre-x 0: the image's sample region is empty"


@pytest.mark.parametrize("alpha,gamma", [(0.25, 2.0), (0.5, 1.5), (-1.0, 2.0), (0.25, 0.0)])
def test_focal_restatement_and_gradient_equal_autograd(alpha, gamma):
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(400, 7, generator=g, dtype=torch.float64) * 6).requires_grad_(True)
    t = torch.rand(400, 7, generator=g) < 0.2
    want = FR.focal_fvcore(z, t, alpha, gamma)
    (grad,) = torch.autograd.grad(want.sum(), z)
    loss, gr = FR.focal(z.detach(), t, alpha, gamma)
    assert float((loss - want.detach()).abs().max()) <= 1e-12
    assert float((gr - grad).abs().max()) <= 1e-12


def _codes(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 256, 1, 1, generator=g), torch.randn(n, generator=g)


def test_optimizer_follows_sgd_normaliser_mask_and_schedule():
    from sylph_amd.finetune import CodeOptimizer
    w0, b0 = _codes(6)
    mask = [True, False, True, True, False, True]
    opt = CodeOptimizer(w0, b0, lr=0.1, momentum=0.9, weight_decay=1e-2, trainable=mask, lr_steps=(2, 4), lr_gamma=0.5)
    w, b, bw, bb = w0.reshape(6, 256).clone(), b0.clone(), None, None
    g = torch.Generator().manual_seed(1)
    lrs = []
    for it, npos in enumerate([7, 0, 3, 11, 1]):
        gw, gb = torch.randn(6, 256, generator=g), torch.randn(6, generator=g)
        lrs.append(opt.lr)
        norm = opt.step(gw.clone(), gb.clone(), torch.tensor([npos], dtype=torch.int32))
        assert float(norm) == max(npos, 1)
        lr = 0.1 * 0.5 ** sum(it >= s for s in (2, 4))
        w, bw = FR.sgd_ref(w, gw / max(npos, 1), bw, lr, 0.9, 1e-2)
        b, bb = FR.sgd_ref(b, gb / max(npos, 1), bb, lr, 0.9, 1e-2)
        tr = torch.tensor(mask)
        assert torch.allclose(opt.w[tr], w[tr], rtol=1e-6, atol=1e-7) and torch.allclose(opt.b[tr], b[tr], rtol=1e-6, atol=1e-7)
        assert torch.equal(opt.w[~tr], w0.reshape(6, 256)[~tr]) and torch.equal(opt.b[~tr], b0[~tr]), "a frozen row moved"
    assert lrs == pytest.approx([0.1, 0.1, 0.05, 0.05, 0.025])


def test_step_records_reads_every_record_before_repeating():
    from sylph_amd.finetune import step_records
    assert step_records(3, None, 2, 0) == [[0, 1, 2]] * 2
    plan = step_records(6, 2, 6, seed=4)
    assert plan == step_records(6, 2, 6, seed=4) and plan != step_records(6, 2, 6, seed=5)
    assert sorted(sum(plan[:3], [])) == list(range(6)) and sorted(sum(plan[3:], [])) == list(range(6))


def test_refusals_by_name(monkeypatch):
    from sylph_amd import distributed as D
    from sylph_amd import finetune as FT
    w, b = _codes(4)
    with pytest.raises(ValueError, match="3x3 class codes are not supported"):
        FT.CodeOptimizer(torch.zeros(4, 256, 3, 3), b, lr=0.1)
    with pytest.raises(ValueError, match="trainable has 3 entries for 4 classes"):
        FT.CodeOptimizer(w, b, lr=0.1, trainable=[True] * 3)
    with pytest.raises(ValueError, match="5 biases for 4 classes"):
        FT.CodeOptimizer(w, torch.zeros(5), lr=0.1)
    with pytest.raises(ValueError, match="records_per_step 4 with 3 records"):
        FT.step_records(3, 4, 1, 0)
    ann = [{"boxes": torch.zeros(1, 4), "classes": torch.tensor([4]), "image_index": torch.tensor([0])}]
    with pytest.raises(ValueError, match="record 0 has a label >= N"):
        FT._check_annotations(ann, [None], 4)
    with pytest.raises(ValueError, match="2 annotations for 1 records"):
        FT._check_annotations(ann * 2, [None], 4)

    class Eng:  # never touched: the refusal comes first
        def __getattr__(self, name):
            raise AssertionError(f"engine.{name} used")
    monkeypatch.setattr(D, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="finetune_class_codes.*world size is 2"):
        FT.finetune_class_codes(Eng(), [None], ann, {"cls_conv": w, "cls_bias": b}, iters=1, lr=0.1)
