"""Golden vectors for 3x3 class codes (MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER = ["", "", 3]) from the REFERENCE's own modules
(imported through tests/golden/ref_shim.py, with the helpers of gen_goldens.py).  Run in the build container:

    python tests/golden/gen_spatial_codes_golden.py

Writes tests/golden/g10_spatial_codes.npz (data only).  Inputs that other fixtures already hold are NOT stored again: the support
features and boxes are g3_codegen.npz's (`s{S}_feat{l}_q8`, `s{S}_boxes`), the query pyramid is g1_head_decode.npz's (`feat{l}_q8`);
both are regenerated here from their seeds and asserted equal.  Weights are regenerated from sylph_amd.synthetic seeds and guarded
by checksums.

  support   S in {1, 2, 5} shots of one class -> (1, 256, 3, 3) codes: raw, normalised (forward_normalize_code), formatted
            (format_class_codes_shared of the shuffled records); `ws_*`: WEIGHT_LAYER + SCALE_LAYER, `l2_*`: BIAS_L2_NORM
  head      MetaFCOS.fcos_head on the 2-image 128 x 160 pyramid with N in {1, 5, 20} 3x3 codes -> logits per level; reg / ctr / iou
            of the same head (they do not depend on the codes)
  decode    predict_proposals for N = 5 and for the nine one-tap classes `tap9` (class t is non-zero at tap t = 3 ky + kx only: a
            swapped ky / kx, or a convolution instead of a cross-correlation, moves whole classes)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_goldens as G  # noqa: E402  (installs ref_shim, puts the repo and the package on sys.path)

from spatial_codes_ref import one_tap_codes, spatial_codes  # noqa: E402  (synthetic inputs shared with the tests)
from sylph_amd import synthetic as W  # noqa: E402


def spatial_cfg(lvis=False):
    cfg = G.make_cfg(lvis)
    cfg.MODEL.META_LEARN.CODE_GENERATOR.CLS_LAYER = ["", "", 3]
    if lvis:  # only BIAS_L2_NORM differs from the COCO settings here
        cfg.MODEL.FCOS.NUM_CLASSES = 60
        cfg.MODEL.FCOS.POST_NMS_TOPK_TEST = 100
    return cfg


def support_inputs(S, g3):
    from ref_shim import Boxes, Instances
    H, Wd = 192, 256
    feats = G.feature_pyramid(S, H, Wd, seed=100 + S)
    for l, f in enumerate(feats):
        assert np.array_equal(G.q8(f), g3[f"s{S}_feat{l}_q8"])  # g3's inputs, not stored again
    boxes = torch.from_numpy(g3[f"s{S}_boxes"])
    insts = []
    for i in range(S):
        it = Instances((H, Wd))
        it.gt_boxes = Boxes(boxes[i:i + 1])
        it.gt_classes = torch.tensor([3])
        insts.append(it)
    return feats, insts


def gen_support(out):
    from sylph.modeling.code_generator.code_generator import CodeGenerator
    from sylph.evaluation.meta_learn_evaluation import format_class_codes_shared
    g3 = np.load(os.path.join(HERE, "g3_codegen.npz"))
    for tag, lvis, ws, shots in (("sup", False, False, (1, 2, 5)), ("ws", False, True, (2, 5)), ("l2", True, False, (2, 5))):
        cfg = spatial_cfg(lvis)
        cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
        if ws:
            cg.WEIGHT_LAYER = ["", "", 1]
            cg.SCALE_LAYER = ["", "", 1]
        sd = W.codegen_state_dict(seed=2, weight_scale_layers=ws)
        out[f"{tag}_weights_checksum"] = G.checksum(sd, "code_generator")
        gen = CodeGenerator(cfg, 256, 5, cfg.MODEL.FCOS.FPN_STRIDES).eval()
        missing = G.load_prefixed(gen, sd, "code_generator")
        assert not [m for m in missing if "support_set_cls" in m], missing
        recs = []
        for S in shots:
            feats, insts = support_inputs(S, g3)
            with torch.no_grad():
                code = gen(feats, insts)
            assert tuple(code["cls_conv"].shape) == (1, 256, 3, 3), code["cls_conv"].shape
            for k, v in code.items():
                out[f"{tag}_s{S}_{k}"] = v.numpy()
            recs.append({"support_set_target": torch.tensor(len(recs)), "class_name": f"c{S}",
                         "class_code": {k: v.clone() for k, v in code.items()}})
            print("support", tag, S, code["cls_conv"].flatten()[:3], code["cls_bias"].flatten())
        with torch.no_grad():
            normed = gen(None, None, cls_norm=True, class_codes=recs)
        for S, c in zip(shots, normed):
            out[f"{tag}_s{S}_norm_cls_conv"] = c["class_code"]["cls_conv"].numpy()
            out[f"{tag}_s{S}_norm_cls_bias"] = c["class_code"]["cls_bias"].numpy()
        out[f"{tag}_tap_norms"] = torch.stack([c["class_code"]["cls_conv"].norm(dim=1).reshape(-1) for c in normed]).numpy()
        if tag == "sup":
            fm = format_class_codes_shared([normed[2], normed[0], normed[1]], "cpu")
            out["sup_fmt_cls_conv"] = fm["cls_conv"].numpy()
            out["sup_fmt_cls_bias"] = fm["cls_bias"].numpy()
            print("formatted", tuple(fm["cls_conv"].shape), tuple(fm["cls_bias"].shape))


def gen_head(out):
    from sylph.modeling.meta_fcos.fcos import MetaFCOS
    from ref_shim import ShapeSpec
    cfg = spatial_cfg()
    sd = W.head_state_dict(seed=1, num_classes=60)
    shapes = {f"p{l}": ShapeSpec(channels=256, stride=2 ** l) for l in range(3, 8)}
    model = MetaFCOS(cfg, shapes).eval()
    G.load_prefixed(model, sd, "proposal_generator")
    out["head_weights_checksum"] = G.checksum(sd, "proposal_generator")
    H, Wd, B = 128, 160, 2
    feats = G.feature_pyramid(B, H, Wd, seed=11)
    g1 = np.load(os.path.join(HERE, "g1_head_decode.npz"))
    for l, f in enumerate(feats):
        assert np.array_equal(G.q8(f), g1[f"feat{l}_q8"])  # g1's pyramid, not stored again
    image_sizes = [(H, Wd - 7), (H - 5, Wd)]
    out["image_sizes"] = np.array(image_sizes)
    cases = [(f"n{n}", spatial_codes(n, seed=60 + n, scale=sc)) for n, sc in ((1, 1.2), (5, 1.0), (20, 0.8))]
    cases.append(("tap9", one_tap_codes(seed=69, scale=2.5)))
    with torch.no_grad():
        locations = model.compute_locations(feats)
        for tag, codes in cases:
            out[f"{tag}_cls_conv"] = codes["cls_conv"].numpy()
            out[f"{tag}_cls_bias"] = codes["cls_bias"].numpy()
            logits, reg, ctr, iou, _, _ = model.fcos_head(feats, None, False, codes)
            for l in range(5):
                out[f"{tag}_logits{l}"] = logits[l].numpy()
                if tag == "n1":
                    out[f"reg{l}"], out[f"ctr{l}"], out[f"iou{l}"] = reg[l].numpy(), ctr[l].numpy(), iou[l].numpy()
                    assert np.array_equal(out[f"reg{l}"], g1[f"reg{l}"])  # the bbox branch does not see the codes
            props = model.fcos_outputs.predict_proposals(logits, reg, ctr, iou, locations, image_sizes, [])
            out[f"{tag}_count"] = np.array([len(p) for p in props])
            if tag in ("n5", "tap9"):
                for i, p in enumerate(props):
                    out.update(G.inst_to_np(p, f"{tag}_img{i}"))
            print("head", tag, [len(p) for p in props], float(logits[0].max()))


if __name__ == "__main__":
    torch.manual_seed(0)
    np.random.seed(0)
    out = {}
    gen_support(out)
    gen_head(out)
    path = os.path.join(HERE, "g10_spatial_codes.npz")
    np.savez_compressed(path, **out)
    print("done", os.path.getsize(path), "bytes")
