"""Meta-training of the code generator without a GPU: the float64 restatement of tests/codegen_train_ref.py against the reference's own
CodeGenerator in training mode (tests/golden/g14*.npz, written by tests/golden/gen_codegen_train_golden.py), its hand-written backward
against torch autograd with and without the kernels' roundings, and the host logic of sylph_amd/metatrain.py."""
import os

import numpy as np
import pytest
import torch

import codegen_train_ref as R

FILES = {"g14_codegen_train.npz": ["c3s4_gn1_d2_b1", "c3s4_nn1_d2_b1", "c3s4_nn0_d2_b1", "c3s4_gn1_d0_b0"],
         "g14b_codegen_train_s1.npz": ["c2s1_gn1_d2_b1", "c2s1_nn1_d2_b1", "c2s1_nn0_d2_b1", "c2s1_gn1_d0_b0"],
         "g14c_codegen_train_mix.npz": ["c3s4_gn1_d0_b1", "c3s4_gn1_d2_b0"]}
EPISODES = {"c3s4": (3, 4), "c2s1": (2, 1)}


def parse_tag(tag):
    ep, v, d, b = tag.split("_")
    return ep, dict(tower_layers=int(d[1]), has_bias=b[1] == "1", post_norm=v[:2] == "gn", conv_l2_norm=v[2] == "1")


def state_dict64(depth, seed=2):
    from sylph_amd import synthetic as W
    return {k: v.double() for k, v in W.codegen_state_dict(seed=seed, tower_layers=depth).items()}


@pytest.mark.parametrize("fname,tag", [(f, t) for f, tags in FILES.items() for t in tags])
def test_restatement_reproduces_the_reference(golden_dir, fname, tag):
    """Both sides are float64: codes and every parameter gradient within 1e-12 max|golden| per tensor (another summation order).  The
    reference keeps conv_scale.scale / bias_scale.scale as float32 parameters (detectron2's Scale), so autograd rounds THEIR gradient to
    float32: those two are held to 2^-24 |golden|, the reference's own rounding."""
    g = np.load(os.path.join(golden_dir, fname))
    ep, kw = parse_tag(tag)
    n, shot = EPISODES[ep]
    sd = state_dict64(kw["tower_layers"])
    checksum = lambda d: float(sum(v.abs().sum() for k, v in sorted(d.items()) if k.startswith("code_generator")))
    assert abs(checksum(sd) - float(g[f"weights_checksum_d{kw['tower_layers']}"])) < 1e-6
    maps = torch.from_numpy(g[f"{ep}_maps_q8"].astype(np.float64) / 32.0)
    assert maps.shape == (n * shot, 256, 7, 7) and float(maps.min()) >= 0 and float(maps.max()) < 4
    code, bias, sv = R.forward(maps, sd, [shot] * n, **kw)
    for got, key in ((code, "cls_conv"), (bias, "cls_bias")):
        want = torch.from_numpy(g[f"{tag}_{key}"])
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), key
    grads = R.backward(sd, sv, torch.from_numpy(g[f"{ep}_G"]), torch.from_numpy(g[f"{ep}_Gb"]), **kw)
    keys = R.layout_keys(**kw)
    stored = sorted(k.split("grad/")[1] for k in g.files if k.startswith(tag + "_grad/") and not k.endswith(("/sum", "/abs")))
    assert sorted(keys) == stored, "the restatement's layout is the reference's set of trainable tensors"
    for k in keys:
        raw = g[f"{tag}_grad/{k}"]
        want, got = torch.from_numpy(raw).double(), grads[k]
        if got.dim() == 4 and got.shape[0] == 256:
            s, a = float(g[f"{tag}_grad/{k}/sum"]), float(g[f"{tag}_grad/{k}/abs"])
            assert abs(float(got.sum()) - s) <= 1e-12 * a and abs(float(got.abs().sum()) - a) <= 1e-12 * a, k
            got = got[::8, ::8]
        tol = 2.0 ** -24 if raw.dtype == np.float32 else 1e-12
        assert raw.dtype == np.float64 or k.endswith(".scale")
        assert float(want.abs().max()) > 0
        assert float((got.reshape(want.shape) - want).abs().max()) <= tol * float(want.abs().max()), k


@pytest.mark.parametrize("rounding", [False, True])
@pytest.mark.parametrize("depth", [0, 1, 2])
@pytest.mark.parametrize("variant", [(True, True), (False, True), (False, False)])
@pytest.mark.parametrize("has_bias", [True, False])
def test_derivative_against_autograd(rounding, depth, variant, has_bias):
    """the hand-written backward equals torch autograd of the forward, float64, ragged segments; with rounding the forward rounds at the
    kernels' points and both treat every rounding as the identity"""
    kw = dict(tower_layers=depth, has_bias=has_bias, post_norm=variant[0], conv_l2_norm=variant[1])
    sd = {k: v.clone().requires_grad_(True) for k, v in state_dict64(depth, seed=5).items()}
    g = torch.Generator().manual_seed(3)
    x0 = R.rbf(torch.rand(6, 256, 7, 7, generator=g, dtype=torch.float64) * 2.0)
    seg_len = [1, 3, 2]
    Gc = torch.randn(3, 256, generator=g, dtype=torch.float64)
    Gb = torch.randn(3, generator=g, dtype=torch.float64)
    code, bias, sv = R.forward(x0, sd, seg_len, rounding=rounding, **kw)
    keys = R.layout_keys(**kw)
    auto = torch.autograd.grad((code * Gc).sum() + (bias * Gb).sum(), [sd[k] for k in keys])
    with torch.no_grad():
        hand = R.backward({k: v.detach() for k, v in sd.items()}, {k: ([t.detach() for t in v] if isinstance(v, list) and v and torch.is_tensor(v[0]) else
                                                                      (v.detach() if torch.is_tensor(v) else v)) for k, v in sv.items()}, Gc, Gb, **kw)
    for k, a in zip(keys, auto):
        assert float(a.abs().max()) > 0, k
        assert float((hand[k].reshape(a.shape) - a).abs().max()) <= 1e-11 * float(a.abs().max()), k


def test_rounding_points_change_the_forward_only_at_bf16_scale():
    """the emulation is the float64 forward up to bf16 operand roundings: codes within a few 2^-9 relative (flat), not equal"""
    kw = dict(tower_layers=2, has_bias=True, post_norm=True, conv_l2_norm=True)
    sd = state_dict64(2)
    g = torch.Generator().manual_seed(4)
    x0 = R.rbf(torch.rand(4, 256, 7, 7, generator=g, dtype=torch.float64) * 2.0)
    c0, b0, _ = R.forward(x0, sd, [2, 2], **kw)
    c1, b1, _ = R.forward(x0, sd, [2, 2], rounding=True, **kw)
    rel = float((c1 - c0).norm() / c0.norm())
    assert 0 < rel < 5 * 2.0 ** -9


# ------------------------------------------------------------------------------------------------ host logic
def _layout():
    return [("a.weight", 0, 6), ("a.bias", 6, 2), ("b.weight", 8, 4)]


def test_optimizer_frozen_prefixes_keep_their_bits():
    from sylph_amd.metatrain import GeneratorOptimizer
    p0 = torch.arange(12, dtype=torch.float32) / 7.0
    opt = GeneratorOptimizer(p0, _layout(), lr=0.1, momentum=0.9, weight_decay=0.1, clip_norm=None, trainable=["a."])
    for _ in range(3):
        opt.step(torch.ones(12), torch.tensor([2]))
    assert torch.equal(opt.p[8:], p0[8:]) and not torch.equal(opt.p[:8], p0[:8])
    sd = opt.state_dict()
    assert sorted(sd) == ["a.bias", "a.weight", "b.weight"] and torch.equal(sd["b.weight"], p0[8:])
    with pytest.raises(ValueError, match="matches no tensor"):
        GeneratorOptimizer(p0, _layout(), trainable=["c."])
    with pytest.raises(ValueError, match="the layout 12"):
        GeneratorOptimizer(p0[:5], _layout())


def test_optimizer_lr_steps_and_division_by_num_pos():
    from sylph_amd.metatrain import GeneratorOptimizer
    p0 = torch.zeros(12)
    opt = GeneratorOptimizer(p0, _layout(), lr=1.0, momentum=0.0, weight_decay=0.0, clip_norm=None, lr_steps=[2], lr_gamma=0.5)
    g = torch.full((12,), 4.0)
    opt.step(g, torch.tensor([4]))      # p = -1
    assert torch.equal(opt.p, torch.full((12,), -1.0)) and opt.lr == 1.0
    opt.step(g, torch.tensor([0]))      # num_pos 0 counts as 1: p = -5; the LR now halves
    assert torch.equal(opt.p, torch.full((12,), -5.0)) and opt.lr == 0.5
    opt.step(g, torch.tensor([4]))      # p = -5.5
    assert torch.equal(opt.p, torch.full((12,), -5.5))


def test_optimizer_clipping_scales_the_flat_gradient_exactly():
    from sylph_amd.metatrain import GeneratorOptimizer, clip_scale
    g = torch.randn(12, generator=torch.Generator().manual_seed(1)) * 10
    opt = GeneratorOptimizer(torch.zeros(12), _layout(), lr=1.0, momentum=0.0, weight_decay=0.0, clip_norm=1.0)
    opt.step(g, torch.tensor([1]))
    want = g * (1.0 / (g.norm() + 1e-6))
    assert torch.equal(opt.p, -want) and abs(float(opt.p.norm()) - 1.0) < 1e-5
    # torch's own clip_grad_norm_ gives the same factor
    q = torch.zeros(12, requires_grad=True)
    q.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([q], 1.0)
    assert torch.allclose(q.grad, want, rtol=1e-6, atol=0)
    assert float(clip_scale(torch.tensor(0.5), 1.0)) == 1.0  # a small gradient is left alone
    small = GeneratorOptimizer(torch.zeros(12), _layout(), lr=1.0, momentum=0.0, weight_decay=0.0, clip_norm=1.0)
    small.step(g / 1000, torch.tensor([1]))
    assert torch.equal(small.p, -(g / 1000))


def _bank():
    from sylph_amd.metatrain import RoiBank
    b = RoiBank()
    cls = [0] * 5 + [1] * 2 + [2] * 7 + [5] * 4 + [9] * 1
    b.append(torch.zeros(len(cls), 49, 256, dtype=torch.bfloat16), cls)
    return b


def test_roi_bank_draw_is_reproducible_and_skips_short_classes():
    from sylph_amd.metatrain import RoiBank
    b = _bank()
    assert len(b) == 19 and b.nbytes == 19 * 49 * 256 * 2 and b.classes() == [0, 1, 2, 5, 9]
    seen = set()
    for seed in range(40):
        idx, seg_len, cids = b.draw(2, 4, seed)
        assert (idx, seg_len, cids) == b.draw(2, 4, seed)
        assert seg_len == [4, 4] and cids == sorted(cids) and set(cids) <= {0, 2, 5}, "classes 1 and 9 hold fewer than 4 rows"
        for j, c in enumerate(cids):
            rows = idx[4 * j:4 * j + 4]
            assert len(set(rows)) == 4 and all(b.class_ids[r] == c for r in rows)
        seen.add(tuple(cids))
    assert len(seen) == 3, "every pair of the three able classes is drawn over 40 seeds"
    with pytest.raises(ValueError, match="cannot be drawn"):
        b.draw(4, 4, 0)
    with pytest.raises(ValueError, match="at least 1"):
        b.draw(0, 4, 0)
    with pytest.raises(ValueError, match=r"\(49, 256\) bf16"):
        b.append(torch.zeros(2, 49, 256), [0, 0])
    both = RoiBank.cat([b, _bank()])
    assert len(both) == 38 and both.rows_of(9) == [18, 37] and both.tensor().shape == (38, 49, 256)


def test_episode_annotations_filter_and_renumber():
    from sylph_amd.metatrain import episode_annotations
    ann = {"boxes": torch.arange(20, dtype=torch.float32).reshape(5, 4), "classes": torch.tensor([7, 3, 9, 3, 11]), "image_index": torch.tensor([0, 0, 1, 1, 1])}
    bx, cl, im = episode_annotations(ann, [3, 9, 20])
    assert cl.tolist() == [0, 1, 0] and im.tolist() == [0, 1, 1] and torch.equal(bx, ann["boxes"][[1, 2, 3]])
    bx, cl, im = episode_annotations(ann, [100])
    assert bx.shape == (0, 4) and cl.numel() == 0 and im.numel() == 0
    with pytest.raises(ValueError, match="image indices"):
        episode_annotations({"boxes": torch.zeros(2, 4), "classes": torch.zeros(2), "image_index": torch.zeros(1)}, [0])


class _Model:
    def __init__(self, cfg):
        self.cfg = cfg
        self.engine = None


def _train_cfg(**over):
    from sylph_amd.config import get_default_cfg
    cfg = get_default_cfg()
    cfg.MODEL.PROPOSAL_GENERATOR.FREEZE_CLS_TOWER = True
    for k, v in over.items():
        cfg.merge_from_list([k, v])
    return cfg


@pytest.mark.parametrize("over,match", [
    ({"MODEL.META_LEARN.CODE_GENERATOR.CONTRASTIVE_LOSS": "snnl"}, "CONTRASTIVE_LOSS"),
    ({"MODEL.META_LEARN.CODE_GENERATOR.DISTILLATION_LOSS_WEIGHT": 0.5}, "DISTILLATION_LOSS_WEIGHT"),
    ({"MODEL.PROPOSAL_GENERATOR.FREEZE_CLS_TOWER": False}, "FREEZE_CLS_TOWER"),
])
def test_train_refuses_by_name(over, match):
    from sylph_amd.metatrain import train_code_generator
    with pytest.raises(NotImplementedError, match=match):
        train_code_generator(_Model(_train_cfg(**over)), _bank(), [], [], iters=1, classes_per_step=2, shots=4)


def test_train_refuses_multi_rank_runs(monkeypatch):
    from sylph_amd import distributed as D
    from sylph_amd.metatrain import train_code_generator
    monkeypatch.setattr(D, "get_world_size", lambda: 2)
    with pytest.raises(NotImplementedError, match="world size is 2"):
        train_code_generator(_Model(_train_cfg()), _bank(), [], [], iters=1, classes_per_step=2, shots=4)


def test_shot_bank_stamp_is_checked_by_name():
    from sylph_amd.shots import ShotBank

    class Eng:
        stamp = 0

        def codegen_stamp(self):
            return self.stamp
    bank = ShotBank({"generator": "CodeGenerator", "code_ksize": 1, "dtype": "bf16", "row_floats": 260})
    eng = Eng()
    assert bank.stamp == 0
    bank.check_stamp(eng)
    eng.stamp = 3
    with pytest.raises(ValueError, match="generator stamp 0, the engine now runs stamp 3"):
        bank.check_stamp(eng)
    eng.stamp = 0
    bank.check_stamp(eng)
