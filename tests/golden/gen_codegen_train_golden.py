"""Golden codes and parameter gradients from the REFERENCE's own CodeGenerator in training mode (imported through tests/golden/ref_shim.py,
with the helpers of gen_goldens.py).  Run in the build container:

    python tests/golden/gen_codegen_train_golden.py

Writes data only.  The reference CodeGenerator(...).train() runs under torch.set_default_dtype(torch.float64) with its box_pooler replaced
by a module that returns fixed ROI maps; weights are synthetic.codegen_state_dict(seed=2) (checksum stored, as in g3).  Three files, each
below the size limit of a committed file:

  g14_codegen_train.npz        3 classes x 4 shots: (POST_NORM, CONV_L2_NORM) = ("GN", on), ("", on), ("", off) at tower depth 2 with a
                               BIAS_LAYER; depth 0 without one
  g14b_codegen_train_s1.npz    2 classes x 1 shot: the same four cases
  g14c_codegen_train_mix.npz   3 classes x 4 shots: depth 0 with a BIAS_LAYER, depth 2 without one (("GN", on))

Keys, per case tag {episode}_{pn}{l2}_d{depth}_b{bias}:
  {episode}_maps_q8                      the ROI maps (M, 256, 7, 7), multiples of 1/32 in [0, 4) as int8
  {episode}_G, {episode}_Gb              the fixed upstream gradient of the codes (n, 256) and of the biases (n)
  {tag}_cls_conv (n, 256), {tag}_cls_bias (n)   the train-mode outputs
  {tag}_grad/{key}                       autograd's gradient of sum(code * G) + sum(bias * Gb): whole for every vector and scalar parameter;
                                         for a (256, 256, 3, 3) tensor the sub-lattice [::8, ::8] with {key}/sum and {key}/abs, its float64
                                         sum and sum of absolute values
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_goldens as G  # noqa: E402  (installs ref_shim, puts the repo and the package on sys.path)

EPISODES = {"c3s4": (3, 4, 141), "c2s1": (2, 1, 142)}
VARIANTS = (("GN", True), ("", True), ("", False))
P = "code_generator"


def tag_of(ep, pn, l2, depth, bias):
    return f"{ep}_{'gn' if pn else 'nn'}{int(l2)}_d{depth}_b{int(bias)}"


def episode_inputs(ep):
    n, shot, seed = EPISODES[ep]
    g = torch.Generator().manual_seed(seed)
    maps = torch.randint(0, 128, (n * shot, 256, 7, 7), generator=g).to(torch.float64) / 32.0
    Gc = torch.randn(n, 256, generator=g, dtype=torch.float64)
    Gb = torch.randn(n, generator=g, dtype=torch.float64)
    return maps, Gc, Gb


class FixedMaps(torch.nn.Module):
    def __init__(self, maps):
        super().__init__()
        self.maps = maps

    def forward(self, features, boxes):
        return self.maps


def run_case(out, ep, pn, l2, depth, bias):
    from sylph.modeling.code_generator.code_generator import CodeGenerator
    from ref_shim import Boxes, Instances
    from sylph_amd import synthetic as W
    n, shot, _ = EPISODES[ep]
    maps, Gc, Gb = episode_inputs(ep)
    cfg = G.make_cfg()
    cg = cfg.MODEL.META_LEARN.CODE_GENERATOR
    cg.POST_NORM = pn
    cg.CONV_L2_NORM = l2
    cg.TOWER_LAYERS = [["GN", "ReLU"]] * depth
    cg.BIAS_LAYER = ["", "", 1] if bias else []
    cfg.MODEL.META_LEARN.SHOT = shot
    torch.set_default_dtype(torch.float32)  # the checkpoint is float32, as in g3; the reference then runs on it in float64
    sd = W.codegen_state_dict(seed=2, tower_layers=depth)
    torch.set_default_dtype(torch.float64)
    out["weights_checksum_d%d" % depth] = G.checksum(sd, "code_generator")
    gen = CodeGenerator(cfg, 256, 5, cfg.MODEL.FCOS.FPN_STRIDES).train()
    have = {f"{P}.{k}" for k in gen.state_dict()}  # the checkpoint's tensors of heads this config does not build are left out
    G.load_prefixed(gen, {k: v for k, v in sd.items() if k in have}, P)
    head = gen.code_generator_head
    head.box_pooler = FixedMaps(maps)
    insts = []
    for i in range(n * shot):
        it = Instances((64, 64))
        it.gt_boxes = Boxes(torch.tensor([[4.0, 4.0, 40.0, 40.0]]))
        it.gt_classes = torch.tensor([i // shot])
        insts.append(it)
    res = head.forward_roi_align([maps], insts)
    code = res["cls_conv"].reshape(n, 256)
    cbias = res["cls_bias"].reshape(n)
    loss = (code * Gc).sum() + (cbias * Gb).sum()
    names, params = zip(*[(k, p) for k, p in gen.named_parameters() if "init_norm" not in k])
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    tag = tag_of(ep, pn, l2, depth, bias)
    out[f"{ep}_maps_q8"] = G.q8(maps.float())
    out[f"{ep}_G"] = Gc.numpy()
    out[f"{ep}_Gb"] = Gb.numpy()
    out[f"{tag}_cls_conv"] = code.detach().numpy()
    out[f"{tag}_cls_bias"] = cbias.detach().numpy()
    for k, g in zip(names, grads):
        if g is None:
            continue
        key = f"{tag}_grad/{P}.{k}"
        g = g.detach()
        if g.dim() == 4 and g.shape[0] == 256:
            out[key] = g[::8, ::8].contiguous().numpy()
            out[key + "/sum"] = np.array(float(g.sum()))
            out[key + "/abs"] = np.array(float(g.abs().sum()))
        else:
            out[key] = g.numpy()
    print(tag, float(loss.detach()), sorted(k for k, g in zip(names, grads) if g is None))


def write(name, cases):
    out = {}
    for c in cases:
        run_case(out, *c)
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    torch.set_default_dtype(torch.float64)
    for ep, name in (("c3s4", "g14_codegen_train.npz"), ("c2s1", "g14b_codegen_train_s1.npz")):
        write(name, [(ep, pn, l2, 2, True) for pn, l2 in VARIANTS] + [(ep, "GN", True, 0, False)])
    write("g14c_codegen_train_mix.npz", [("c3s4", "GN", True, 0, True), ("c3s4", "GN", True, 2, False)])
