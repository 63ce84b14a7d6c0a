"""Shot bank, host side: the C ABI's three symbols, ShotBank's draws and files, the runner's one-rank refusal, and the float32
restatement of pool + combine (tests/shot_bank_ref.py) against the oracle's code computation.

The restatement follows the KERNEL's order of additions, the oracle (oracle/codegen.py, and tests/spatial_codes_ref.py for the 3 x 3
pooling) torch's, so the two agree within fp32 rounding, not to the bit: |got - want| <= 1e-6 * max |want| per output array.  The
inputs are N(0.5, 1) so that every output has a scale of order 0.1 .. 1 to be relative to; a sum of 49 (or 9) such terms and then of
up to 70 weighted shots carries a rounding error of a few 1e-8 of that scale."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import shot_bank_ref as SB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shot_bank_symbols_declared_and_exported():
    from sylph_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sylph_hip.h")).read()
    declared = set(re.findall(r"\b(sylph_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    c_int, vp, ip = ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
    want = {"sylph_shot_row_floats": [vp, ip], "sylph_codegen_shots": [vp, c_int, vp, ip, vp],
            "sylph_shot_combine": [vp, vp, c_int, c_int, ip, c_int, ip, vp, vp]}
    for name, args in want.items():
        assert name in declared and name in _lib.PROTOTYPES
        assert getattr(L, name) is not None
        assert _lib.PROTOTYPES[name] == (c_int, args)


# ------------------------------------------------------------------------------------------------ ShotBank
KEY = {"generator": "CodeGenerator", "code_ksize": 1, "dtype": "bf16", "row_floats": 260}


def _bank():
    from sylph_amd.shots import ShotBank
    bank = ShotBank(KEY)
    g = torch.Generator().manual_seed(0)
    cls = [5] * 6 + [2] * 2 + [9] * 11 + [2] * 1  # classes 5, 2, 9 with 6, 3 and 11 instances; class 2 in two pieces
    bank.append(torch.randn(8, 260, generator=g), cls[:8], list(range(8)), [0] * 8)
    bank.append(torch.randn(12, 260, generator=g), cls[8:], list(range(8, 20)), [1] * 12)
    return bank, cls


def test_draw_is_deterministic_without_replacement_and_in_class_order():
    bank, cls = _bank()
    assert len(bank) == 20 and bank.nbytes == 20 * 260 * 4 and tuple(bank.tensor().shape) == (20, 260)
    assert bank.rows_of(2) == [6, 7, 19] and bank.classes() == [2, 5, 9]
    for shots in (1, 3, 5, 30):
        idx, seg_len, cids = bank.draw(shots, seed=4)
        assert (idx, seg_len, cids) == bank.draw(shots, seed=4), "not deterministic in (shots, seed)"
        assert cids == [2, 5, 9], "ascending class ids"
        assert seg_len == [min(shots, 3), min(shots, 6), min(shots, 11)]
        i0 = 0
        for c, n in zip(cids, seg_len):
            part = idx[i0:i0 + n]
            assert len(set(part)) == n, "drawn with replacement"
            assert all(cls[r] == c for r in part)
            if n < shots or n == len(bank.rows_of(c)):
                assert part == bank.rows_of(c), "a short class gives all its rows, in bank order"
            i0 += n
        assert i0 == len(idx)
    assert bank.draw(3, seed=4)[0] != bank.draw(3, seed=5)[0]
    # the generator is numpy.random.RandomState(seed), consumed in class order: class 2 has exactly 3 rows and draws nothing
    rng = np.random.RandomState(4)
    want = bank.rows_of(2) + [bank.rows_of(5)[i] for i in rng.choice(6, 3, replace=False)] + [bank.rows_of(9)[i] for i in rng.choice(11, 3, replace=False)]
    assert bank.draw(3, seed=4)[0] == want
    assert bank.draw(2, seed=1, classes=[9, 5])[2] == [5, 9]
    with pytest.raises(ValueError, match="class 7 has no banked instance"):
        bank.draw(2, seed=0, classes=[7])
    with pytest.raises(ValueError, match="260 fp32 floats wide"):
        bank.append(torch.zeros(2, 257), [0, 0], [0, 0], [0, 0])
    with pytest.raises(ValueError, match="2 rows with 1 class ids"):
        bank.append(torch.zeros(2, 260), [0], [0, 0], [0, 0])


def test_save_load_round_trip_and_key_mismatch(tmp_path):
    from sylph_amd.shots import ShotBank
    bank, cls = _bank()
    path = str(tmp_path / "bank.pth")
    bank.save(path)
    raw = torch.load(path)
    assert set(raw) == {"key", "rows", "class_ids", "image_ids", "ann_ids"} and torch.is_tensor(raw["rows"]) and isinstance(raw["class_ids"], list)
    back = ShotBank.load(path)
    assert back.key == bank.key and torch.equal(back.tensor(), bank.tensor())
    assert (back.class_ids, back.image_ids, back.ann_ids) == (bank.class_ids, bank.image_ids, bank.ann_ids)
    assert back.draw(3, 7) == bank.draw(3, 7)

    class Eng:
        device = torch.device("cpu")

        def __init__(self, **kw):
            self.k = dict(KEY, **kw)

        def shot_key(self):
            return self.k

    ShotBank.load(path, engine=Eng())
    for field, other in (("generator", "ROIEncoder"), ("code_ksize", 3), ("dtype", "f32"), ("row_floats", 2308)):
        with pytest.raises(ValueError, match=f"made with {field} = "):
            ShotBank.load(path, engine=Eng(**{field: other}))
        with pytest.raises(ValueError, match=f"made with {field} = "):
            bank.check_key(Eng(**{field: other}))


def test_bank_sweep_is_refused_on_several_ranks(monkeypatch):
    from sylph_amd import distributed as D
    from sylph_amd.runner import MetaFCOSRunner
    bank, _ = _bank()
    monkeypatch.setattr(D, "get_world_size", lambda: 2)

    class Model:  # never touched: the refusal comes first
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} used")

    with pytest.raises(NotImplementedError, match="shot_bank.*world size is 2"):
        MetaFCOSRunner()._do_test_meta_learning(None, Model(), shot_bank=bank, bank_draws=[(1, 0)], query_loader=[])
    monkeypatch.setattr(D, "get_world_size", lambda: 1)
    with pytest.raises(ValueError, match="shot_bank and bank_draws go together"):
        MetaFCOSRunner()._do_test_meta_learning(None, Model(), shot_bank=bank, query_loader=[])


# ------------------------------------------------------------------------------------------------ restatement vs the oracle
def _identity_heads():
    """A code-generator head whose 3 x 3 convs copy their input: cls_conv = the 256 input channels, the bias / shot-weight / class-scale
    heads = input channels 0 / 1 / 2 (centre tap 1, every other weight and every bias 0: the zero products add exactly)."""
    from oracle.codegen import CG_PREFIX
    sd = {}
    w = torch.zeros(256, 256, 3, 3)
    w[torch.arange(256), torch.arange(256), 1, 1] = 1.0
    sd[f"{CG_PREFIX}.support_set_cls_conv.0.weight"], sd[f"{CG_PREFIX}.support_set_cls_conv.0.bias"] = w, torch.zeros(256)
    for ch, name in enumerate(("support_set_cls_bias", "support_set_cls_weight", "support_set_cls_scale")):
        w1 = torch.zeros(1, 256, 3, 3)
        w1[0, ch, 1, 1] = 1.0
        sd[f"{CG_PREFIX}.{name}.0.weight"], sd[f"{CG_PREFIX}.{name}.0.bias"] = w1, torch.zeros(1)
    return sd


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    err, scale = float(np.abs(np.asarray(got, dtype=np.float64) - want).max()), float(np.abs(want).max())
    print(f"{what}: max |diff| {err:.3e}, scale {scale:.3e}")
    assert err <= 1e-6 * scale, f"{what}: {err} > 1e-6 * {scale}"


@pytest.mark.parametrize("S", [1, 5, 70])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("weight_scale,bias_l2", [(False, False), (True, False), (False, True), (True, True)])
def test_restatement_agrees_with_the_oracle(weight_scale, bias_l2, k, S):
    from oracle import codegen as CG
    import spatial_codes_ref as SC
    g = torch.Generator().manual_seed(1000 * S + 10 * k + 2 * weight_scale + bias_l2)
    roi = torch.randn(S, 256, 7, 7, generator=g) + 0.5
    kw = dict(tower_spec=[], bias_l2_norm=bias_l2, has_weight_layer=weight_scale, has_scale_layer=weight_scale)
    want = CG.code_from_roi_features(roi, _identity_heads(), **kw) if k == 1 else SC.code_from_roi_features(roi, _identity_heads(), k=3, **kw)
    conv = roi.numpy()
    rows = SB.pool_rows(conv, conv[:, :3], ib=0, iw=1 if weight_scale else -1, is_=2 if weight_scale else -1, k=k, bias_l2_norm=bias_l2)
    assert rows.shape == (S, SB.row_floats(k)) and rows.dtype == np.float32 and np.all(rows[:, -1] == 0)
    if not weight_scale:
        assert np.all(rows[:, -3:-1] == 0), "an absent head writes 0"
    # a permuted, partly repeated index list over a bank that holds the shots in another order: the gather is part of what is restated
    perm = np.random.RandomState(S).permutation(S)
    bank = np.concatenate([rows[perm], rows[:1] * 0 + 7])  # (a last row nobody draws)
    inv = np.argsort(perm)
    codes, wn = SB.combine_rows(bank, list(inv), [S], k=k, softmax=weight_scale)
    n = 256 * k * k
    _close(codes[0, :n], want["cls_conv"].reshape(-1).numpy(), "cls_conv")
    _close(codes[0, n:], want["cls_bias"].reshape(-1).numpy(), "cls_bias")
    if weight_scale:
        _close(wn, want["cls_weight_norm"].reshape(-1).numpy(), "cls_weight_norm")
    # two segments in one list are the two codes: nothing crosses a segment
    if S >= 5:
        two, _ = SB.combine_rows(bank, list(inv[:2]) + list(inv), [2, S], k=k, softmax=weight_scale)
        assert np.array_equal(two[1], codes[0])
        one, _ = SB.combine_rows(bank, list(inv[:2]), [2], k=k, softmax=weight_scale)
        assert np.array_equal(two[0], one[0])


def test_restated_tree_and_mean():
    v = np.arange(64, dtype=np.float32)
    assert SB.xor_tree(v) == np.float32(2016)
    rows = np.random.RandomState(0).randn(6, 260).astype(np.float32)
    m = SB.mean_rows(rows, [4, 4, 1, 0], [3, 1])
    assert np.array_equal(m[1], rows[0, :256])
    assert np.array_equal(m[0], ((rows[4, :256] + rows[4, :256]) + rows[1, :256]) / np.float32(3))
