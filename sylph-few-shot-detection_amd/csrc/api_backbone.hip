// Host side of libsylph_hip.so, unit "backbone": input pipeline + ResNet-FPN stage (sylph_preprocess*, sylph_backbone_fpn, pyramid import / export).
// No torch types, no CPU compute fallback: every stage is a HIP kernel from this directory.
#include "api_internal.h"

namespace sylph_host {

std::shared_ptr<PilCoeffs> pil_bilinear_coeffs(int in_size, int out_size) {
  auto pc = std::make_shared<PilCoeffs>();
  const double scale = (double)in_size / (double)out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 1.0 * filterscale;  // bilinear filter support = 1
  const int ksize = (int)ceil(support) * 2 + 1;
  pc->ksize = ksize;
  pc->bounds.assign((size_t)out_size * 2, 0);
  pc->kk.assign((size_t)out_size * ksize, 0);
  std::vector<double> k((size_t)ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double a = (x + xmin - center + 0.5) * ss;
      if (a < 0.0) a = -a;
      const double w = a < 1.0 ? 1.0 - a : 0.0;
      k[x] = w;
      ww += w;
    }
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) k[x] /= ww;
      pc->kk[(size_t)xx * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (double)(1 << 22)) : (int)(0.5 + k[x] * (double)(1 << 22));
    }
    pc->bounds[2 * xx] = xmin;
    pc->bounds[2 * xx + 1] = xmax;
  }
  return pc;
}

int ensure_pyramid(sylph_ctx* c, Plan* P) {
  if (!P->F) RET(c->dalloc(&P->F, (size_t)P->B * P->Ltot * 256 * c->esz()));
  return 0;
}

// One launch of a kernel that walks a patch table (bottleneck.hip, conv_rw3.hip, conv_rw64.hip), appended to `ops`: the table of the
// ph x pw patches of B images of H x W positions is uploaded and handed to the kernel in a.bk / a.n_tiles
// even_rp != 0: the stride-2-output form (BkTile): ph x pw tiles of the H/2 x W/2 output map, t1 row pitch even_rp
template <typename Args>
static int add_patch_kernel(sylph_ctx* c, std::vector<OpFn>& ops, const char* kern, double flops, int (*launch)(const Args&, hipStream_t), Args a,
                            int B, int H, int W, int ph, int pw, int even_rp = 0) {
  std::vector<BkTile> bt;
  for (int b = 0; b < B; ++b) {
    if (even_rp) {
      for (int yy = 0; yy < H / 2; yy += ph)
        for (int xx = 0; xx < W / 2; xx += pw)
          bt.push_back(BkTile{b * H * W, H, W, (yy << 16) | xx, ph | (even_rp << 16), pw, (65536u + pw - 1) / pw, (65536u + 2 * pw) / (2 * pw + 1)});
      continue;
    }
    for (int yy = 0; yy < H; yy += ph)
      for (int xx = 0; xx < W; xx += pw)
        bt.push_back(BkTile{b * H * W, H, W, (yy << 16) | xx, ph, pw, (65536u + pw - 1) / pw, (65536u + pw + 2 - 1) / (pw + 2)});
  }
  void* btd = nullptr;
  RET(upload(c, &btd, bt.data(), bt.size() * sizeof(BkTile)));
  a.bk = (const BkTile*)btd;
  a.n_tiles = (int)bt.size();
  ops.push_back([=](hipStream_t s) { return timed_op(c, kern, flops, s, [=](hipStream_t st) { return launch(a, st); }); });
  return 0;
}

// Below this many patches a launch of conv_rw64 (one persistent block per CU, weights loaded into registers first) is left to the
// generic route.  Measured at 200 x 336 (272 patches per image, profiles/resnet_basic_conv64.txt): 1 image a tie, 2 and 4 images
// (544 / 1 088 patches: 3 and 5 rounds over the 256 CUs, the last one nearly empty) 4-28 % behind conv_igemm's 64-row tiles, 8 images
// (2 176) 3-14 % ahead, 64 and 192 images 1.4-1.55 x.
static const long RW64_MIN_PATCHES = 2048;

// The kernel of one dense 3x3 pad-1 conv L + FrozenBN [+ residual] [+ ReLU] on B images of H x W (Conv3Route).  Both dedicated kernels
// are bf16, stride 1, and need the layer's scale and shift:
//   conv_rw3   128 -> 128, FrozenBN + ReLU without a residual (the callers ask for layers with that epilogue only): res3 conv2 of the bottleneck nets, conv1 of
//              the res3 identity BasicBlocks.  Launches of at least 256 x 120 positions; 800 x 1344: 100 x 168 -> 10 x 12 patches (halo
//              12 x 14 = 168 rows).  SYLPH_CONV_RW3: 0 off, 2 any launch.
//   conv_rw64  64 -> 64: the res2 convs of R-18 / R-34.  Launches of at least RW64_MIN_PATCHES patches; 200 x 336 -> 12 x 21 patches (halo
//              14 x 23 = 322 pixels).  SYLPH_CONV_RW64: 0 off, 2 any launch; read per pick so that one process can build both.
Conv3Route pick_conv3_route(const sylph_ctx* c, const ConvLayer& L, int B, int H, int W, int stride) {
  Conv3Route r;
  if (c->dt != DT_BF16 || L.groups != 1 || L.KH != 3 || L.KW != 3 || stride != 1 || !L.scale || !L.shift) return r;
  const size_t pos = (size_t)B * H * W;
  int ph = 0, pw = 0;
  if (const int on = knob::conv_rw3(); on && L.Cin == 128 && L.Cout == 128 && L.Cout_pad == 128 &&
      pos * 256 < ((size_t)1 << 31) &&  // (2 GiB buffer descriptors)
      (on == 2 || pos >= (size_t)256 * 120)) {
    pick_patch(H, W, 128, 184, 2, &ph, &pw);
    if (conv_rw3_patch_ok(ph, pw)) { r.kind = Conv3Kind::rw3; r.ph = ph; r.pw = pw; }
    return r;
  }
  if (const int on = knob::conv_rw64(); on && L.Cin == 64 && L.Cout == 64 && L.Cout_pad == 64 && W < 65536 &&
      pos * 128 <= 0xff000000u) {  // (32-bit byte offsets into descriptors of the tensor's real size)
    pick_patch(H, W, 256, 352, 2, &ph, &pw);
    const long n = (long)B * ((H + ph - 1) / ph) * ((W + pw - 1) / pw);
    if (conv_rw64_patch_ok(ph, pw) && (on == 2 || n >= RW64_MIN_PATCHES)) { r.kind = Conv3Kind::rw64; r.ph = ph; r.pw = pw; }
  }
  return r;
}

// One such conv appended to `ops` by its route: x [B][H * W][Cin] -> y [B][Ho * Wo][Cout] (res: same shape as y)
static int add_conv3x3(sylph_ctx* c, std::vector<OpFn>& ops, const ConvLayer& L, const Conv3Route& r, int B, int H, int W, int stride, const void* x,
                       const void* res, void* y, int relu) {
  switch (r.kind) {
    case Conv3Kind::rw3: {
      if (res || !relu) return fail("internal: conv_rw3 is conv + FrozenBN + ReLU");
      BottleneckArgs ba;
      memset(&ba, 0, sizeof(ba));
      ba.x = x; ba.y = y;
      ba.w2 = (const __bf16*)L.w; ba.s2 = L.scale; ba.b2 = L.shift;
      return add_patch_kernel(c, ops, "conv_rw3_kernel", 2.0 * (double)B * H * W * 128.0 * 1152.0, launch_conv_rw3, ba, B, H, W, r.ph, r.pw);
    }
    case Conv3Kind::rw64: {
      ConvRw64Args ra;
      memset(&ra, 0, sizeof(ra));
      ra.x = x; ra.y = y; ra.res = res; ra.w = (const __bf16*)L.w; ra.scale = L.scale; ra.shift = L.shift;
      ra.bytes = (unsigned)((size_t)B * H * W * 128); ra.relu = relu ? 1 : 0;
      return add_patch_kernel(c, ops, "conv_rw64_kernel", 2.0 * (double)B * H * W * 64.0 * 576.0, launch_conv_rw64, ra, B, H, W, r.ph, r.pw);
    }
    case Conv3Kind::generic: break;
  }
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  ConvOpts o; o.stride = stride; o.pad = 1; o.relu_nch = relu ? (1 << 30) : 0;
  if (res) { o.res = res; o.res_ld = L.Cout; o.res_mode = 1; }
  return add_conv(c, ops, L, x, L.Cin, y, L.Cout, image_segs(B, H, W, Ho, Wo), o);
}

// One 3x3 stride-1 pad-1 conv 64 -> 64 + FrozenBN [+ residual] [+ ReLU] on dense images x [B][H * W][64] -> y, appended to `ops`:
// conv_rw64.hip or add_conv (pick_conv3_route).  The parity entry sylph_conv3x3_c64; add_basic_block builds its convs the same way.
int add_conv3x3_c64(sylph_ctx* c, std::vector<OpFn>& ops, const ConvLayer& L, int B, int H, int W, const void* x, const void* res, void* y, int relu) {
  return add_conv3x3(c, ops, L, pick_conv3_route(c, L, B, H, W, 1), B, H, W, 1, x, res, y, relu);
}

// The size test of the pair route is the one pick_conv_route applies to the conv3 layer for conv_spw (spw_r1, api_conv.hip): at least 512
// M tiles of 128 rows counted over the whole launch, ceil(B * H * W / 128) -- two per CU of a 256-CU part.  So with the default knob the
// pair kernel takes exactly the launches whose conv3 would have taken conv_spw, and a smaller launch keeps conv_igemm for both layers.
static const long PAIR_MIN_MTILES128 = 512;

// conv3 + residual of `blk` and conv1 of `next` as one launch (conv_spw_pair.hip): bf16, both identity blocks 512 -> 128 -> 512 with a dense
// conv2, stride 1, FrozenBN on both layers, an image within 32-bit byte offsets
static bool block_pair_ok(const sylph_ctx* c, const sylph_ctx::Block& blk, const sylph_ctx::Block& next, int B, int Cin, int Hin, int Win, int stride,
                          int mid, int cout) {
  const int on = knob::block_pair();
  if (!on || c->dt != DT_BF16 || blk.basic || next.basic || blk.has_sc || next.has_sc || blk.c2.groups != 1 || next.c2.groups != 1) return false;
  if (Cin != 512 || cout != 512 || mid != 128 || stride != 1) return false;
  const ConvLayer &c3 = blk.c3, &c1 = next.c1;
  if (c3.Cin != 128 || c3.Cout != 512 || c3.Cout_pad != 512 || c3.KH != 1 || c3.KW != 1 || !c3.scale || !c3.shift) return false;
  if (c1.Cin != 512 || c1.Cout != 128 || c1.Cout_pad != 128 || c1.KH != 1 || c1.KW != 1 || !c1.scale || !c1.shift) return false;
  const long hw = (long)Hin * Win;
  if (hw * 1024 >= (1L << 32) || (long)B * hw >= (1L << 31)) return false;
  return on == 2 || ((long)B * hw + 127) / 128 >= PAIR_MIN_MTILES128;
}

// How one bottleneck block is built (BlockRoute).  Hin x Win is X's map; with BK_IN_COMPACT `stride` is already 1.  next: the block after
// this one in its stage (nullptr: none, or not of interest).
BlockRoute pick_block_route(const sylph_ctx* c, const sylph_ctx::Block& blk, int B, int Cin, int Hin, int Win, int stride, int mid, int cout, int flags,
                            const sylph_ctx::Block* next) {
  BlockRoute r;
  r.chunk = B;
  r.s1 = c->cfg.stride_in_1x1 ? stride : 1; r.s3 = c->cfg.stride_in_1x1 ? 1 : stride;
  r.H1 = (Hin - 1) / r.s1 + 1; r.W1 = (Win - 1) / r.s1 + 1;
  r.Ho = (Hin - 1) / stride + 1; r.Wo = (Win - 1) / stride + 1;
  // (a grouped conv2 -- ResNeXt -- never takes the fused R-50 kernels nor conv_rw3: they compute a dense 3x3)
  const bool dense2 = blk.c2.groups == 1;
  // The two fused res2 kernels (bottleneck.hip), bf16: the two 64-channel intermediates and the second read of x never reach HBM
  // (identity block: 2 048 -> 1 024 B per position).  32-bit byte offsets inside ONE image (64-bit image base).
  const bool fused64 = knob::fuse_bottleneck() && dense2 && c->dt == DT_BF16 && stride == 1 && mid == 64 && cout == 256 && blk.c1.Cout_pad == 64 &&
                       blk.c2.Cout_pad == 64 && (size_t)Hin * Win * 512 < ((size_t)1 << 32) && (size_t)B * Hin * Win < ((size_t)1 << 31);
  const bool fuse_id = fused64 && !blk.has_sc && Cin == 256 && blk.c3.Cout_pad == 256;
  const bool fuse_pr = fused64 && blk.fused_sc && Cin == 64 && blk.c3sc.Cout_pad == 256 && blk.c3sc.Cin == 128 && !blk.c3sc.scale;
  r.tail_ok = fuse_id && (Hin & 1) == 0 && (Win & 1) == 0;
  if ((flags & BK_EVEN_OUT) && !r.tail_ok) {
    r.refuse = "the stride-2-output bottleneck is the fused bf16 identity block (C 256, mid 64) on a map of even height and width";
    return r;
  }
  r.pair_ok = next && block_pair_ok(c, blk, *next, B, Cin, Hin, Win, stride, mid, cout);
  r.pair_out = (flags & BK_PAIR_OUT) != 0;
  r.pair_in = (flags & BK_PAIR_IN) != 0;
  if (r.pair_out && !r.pair_ok) {
    r.refuse = "the block pair launch is conv3 + residual of a bf16 identity block 512 -> 128 -> 512 followed by another such block";
    return r;
  }
  if (r.pair_in && (c->dt != DT_BF16 || blk.has_sc || Cin != 512 || mid != 128 || stride != 1 || !dense2)) {
    r.refuse = "internal: BK_PAIR_IN on a block whose conv1 the pair launch cannot have computed";
    return r;
  }
  if (!dense2) {
    // ResNeXt: the blocks are up to 8x wider than R-50's (X-101-32x8d res3.0: t1 = 512 channels at res2 resolution, 34 M elements per
    // image), so at large batches whole-tensor offsets of the 1x1 kernels (conv_igemm's 31-bit element offsets, conv_pw's 32-bit residual
    // byte offsets) would overflow.  Such a block is built as a sequence of image chunks, each small enough that every tensor of the chunk
    // stays below 2^31 elements; every chunk runs the block's own launches on its slice of the (dense, image-major) buffers.
    const long per_img = std::max({(long)Hin * Win * Cin, (long)r.H1 * r.W1 * mid, (long)r.Ho * r.Wo * mid, (long)r.Ho * r.Wo * cout});
    const int nb = (int)std::min<long>(B, ((1L << 31) - 1) / per_img);
    if (nb < 1) {
      r.refuse = "image too large for the ResNeXt block kernels: " + std::to_string(per_img) + " elements per image";
      return r;
    }
    if (nb < B) {
      const int nch = (B + nb - 1) / nb;
      r.chunk = (B + nch - 1) / nch;
      return r;
    }
  }
  if (fuse_id || fuse_pr) {
    r.form = fuse_pr ? BlockForm::fused_proj : (flags & BK_EVEN_OUT) ? BlockForm::fused_id_even : BlockForm::fused_id;
    return r;
  }
  r.form = BlockForm::chain;
  r.fused_sc = blk.fused_sc;
  if (!dense2) {
    // ResNeXt conv2: grouped 3x3 (stride s3) + FrozenBN + ReLU, conv_group.hip, on the dense images t1 [B][H1 * W1][mid] -> t2
    const int cpg = mid / blk.c2.groups;
    r.conv2 = Conv2Form::grouped;
    if (blk.c2.Cin != mid || blk.c2.Cout != mid || mid % 64 != 0 || cpg < 4 || cpg > 64 || (cpg & (cpg - 1)) != 0)
      r.refuse = "internal: grouped conv2 shape";
    else if ((long)r.H1 * r.W1 * mid >= (1L << 31))
      r.refuse = "image too large for conv_group: " + std::to_string((long)r.H1 * r.W1 * mid) + " elements per image exceed its 31-bit offsets";
    return r;
  }
  // conv_rw3 where the layer picker gives it; a 64-channel conv2 (the res2 blocks with SYLPH_FUSE_BOTTLENECK=0) stays with add_conv:
  // conv_rw64 is the BasicBlock nets' kernel
  const Conv3Route r2 = pick_conv3_route(c, blk.c2, B, r.H1, r.W1, r.s3);
  if (r2.kind == Conv3Kind::rw3) { r.conv2 = Conv2Form::rw3; r.ph = r2.ph; r.pw = r2.pw; }
  return r;
}

// The res3 block-pair launch (conv_spw_pair.hip) appended to `ops`: y = relu(bn3(c3 t2) + x) and t1 = relu(bn1(c1_next y)) on dense
// tensors t2 [B][HW][128], x / y [B][HW][512], t1 [B][HW][128]; uploads the tile table (res3_pair_tiles.h) and, while profiling, pushes the
// route record "spw_pair 64x512+128".  Shared by add_bottleneck (BK_PAIR_OUT) and the parity entry sylph_res3_pair.
int add_res3_pair(sylph_ctx* c, std::vector<OpFn>& ops, const ConvLayer& c3, const ConvLayer& c1_next, int B, int HW, const void* t2, const void* x, void* y,
                  void* t1) {
  const std::vector<PairTile> pt = pair_tiles(B, HW);
  void* ptd = nullptr;
  RET(upload(c, &ptd, pt.data(), pt.size() * sizeof(PairTile)));
  PairArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.t2 = t2; pa.x = x; pa.y = y; pa.t1 = t1;
  pa.w3 = (const __bf16*)c3.w; pa.w1 = (const __bf16*)c1_next.w;
  pa.s3 = c3.scale; pa.b3 = c3.shift; pa.s1 = c1_next.scale; pa.b1 = c1_next.shift;
  pa.tiles = (const PairTile*)ptd; pa.n_tiles = (int)pt.size();
  const double fl = 2.0 * (double)B * HW * (512.0 * 128 + 128.0 * 512);
  ops.push_back([=](hipStream_t s) { return timed_op(c, "conv_spw_kernel_pair", fl, s, [=](hipStream_t st) { return launch_conv_spw_pair(pa, st); }); });
  if (c->prof) c->route_recs.push_back("spw_pair " + std::to_string(PAIR_TILE_ROWS) + "x512+128");
  return 0;
}

// One ResNet bottleneck block (detectron2 BottleneckBlock: 1x1 -> 3x3 -> 1x1, FrozenBN folded, residual / projection shortcut)
// appended to `ops` as pick_block_route says: X [B][Hin*Win][Cin] -> Y [B][Ho*Wo][cout].  t1 / t2 / sc are scratch activations of the stage.
// Shared by build_backbone and the single-block parity entry sylph_bottleneck, so both run the same kernels.
int add_bottleneck(sylph_ctx* c, std::vector<OpFn>& ops, const sylph_ctx::Block& blk, int B, const void* X, int Cin, int Hin, int Win,
                          int stride, int mid, int cout, void* Y, const BkScratch& scr, int flags, const sylph_ctx::Block* next) {
  const BlockRoute r = pick_block_route(c, blk, B, Cin, Hin, Win, stride, mid, cout, flags, next);
  if (!r.refuse.empty()) return fail(r.refuse);
  const DType dt = c->dt;
  const int H1 = r.H1, W1 = r.W1, Ho = r.Ho, Wo = r.Wo;
  void *t1 = scr.t1, *t2 = scr.t2, *sc = scr.sc;
  if (r.chunk < B) {  // (ResNeXt at a large batch) slice by slice, each with its own route
    const size_t e = c->esz();
    for (int b0 = 0; b0 < B; b0 += r.chunk) {
      const int n = std::min(r.chunk, B - b0);
      BkScratch sub{(char*)t1 + (size_t)b0 * H1 * W1 * mid * e, (char*)t2 + (size_t)b0 * Ho * Wo * mid * e,
                    (char*)sc + (size_t)b0 * Ho * Wo * cout * e, scr.trash};
      RET(add_bottleneck(c, ops, blk, n, (const char*)X + (size_t)b0 * Hin * Win * Cin * e, Cin, Hin, Win, stride, mid, cout,
                         (char*)Y + (size_t)b0 * Ho * Wo * cout * e, sub, flags));
    }
    return 0;
  }
  if (r.form != BlockForm::chain) {
    const bool id = r.form != BlockForm::fused_proj;
    BottleneckArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.x = X; ba.y = Y;
    ba.w1 = (const __bf16*)blk.c1.w; ba.w2 = (const __bf16*)blk.c2.w; ba.w3 = (const __bf16*)(id ? blk.c3.w : blk.c3sc.w);
    ba.s1 = blk.c1.scale; ba.b1 = blk.c1.shift; ba.s2 = blk.c2.scale; ba.b2 = blk.c2.shift;
    ba.s3 = id ? blk.c3.scale : nullptr; ba.b3 = id ? blk.c3.shift : blk.c3sc.shift;
    ba.zeros = c->zeros;
    if (!*scr.trash) RET(c->dalloc(scr.trash, (size_t)1024 * 256 * 128));  // per-thread trash slots (grid <= CU count <= 1024)
    ba.trash = *scr.trash;
    int ph, pw;
    if (r.form == BlockForm::fused_id_even) {
      // outputs at (2 i, 2 j) only, compact: conv1 on every position (each one is in some output's 3x3 window), conv2 / conv3 on a quarter
      int rp;
      bottleneck64_even_patch(Hin, Win, &ph, &pw, &rp);
      const double fl = 2.0 * (double)B * ((double)Hin * Win * 256.0 * 64 + (double)(Hin / 2) * (Win / 2) * (64.0 * 576 + 64.0 * 256));
      return add_patch_kernel(c, ops, "bottleneck64_kernel", fl, launch_bottleneck64_even, ba, B, Hin, Win, ph, pw, rp);
    }
    pick_patch(Hin, Win, 128, 184, 2, &ph, &pw);
    const double fl = 2.0 * (double)B * Hin * Win * (id ? (256.0 * 64 + 64.0 * 576 + 64.0 * 256) : (64.0 * 64 + 64.0 * 576 + 128.0 * 256));
    if (id) return add_patch_kernel(c, ops, "bottleneck64_kernel", fl, launch_bottleneck64, ba, B, Hin, Win, ph, pw);
    return add_patch_kernel(c, ops, "bottleneck64p_kernel", fl, launch_bottleneck64p, ba, B, Hin, Win, ph, pw);
  }
  // the producer already dropped the rows a stride-2 1x1 skips: stride is 1 here, the routes are chosen for the strided layer
  const int route_stride = (flags & BK_IN_COMPACT) ? 2 : 0;
  if (!r.pair_in) {  // (else the pair launch of the block before left conv1's output in t1)
    ConvOpts o1; o1.stride = r.s1; o1.relu_nch = 1 << 30; o1.route_stride = route_stride;
    RET(add_conv(c, ops, blk.c1, X, Cin, t1, mid, image_segs(B, Hin, Win, H1, W1), o1));
  }
  switch (r.conv2) {
    case Conv2Form::grouped: {
      GroupConvArgs ga;
      memset(&ga, 0, sizeof(ga));
      ga.x = t1; ga.y = t2; ga.wt = blk.c2.w; ga.scale = blk.c2.scale; ga.shift = blk.c2.shift;
      ga.B = B; ga.C = mid; ga.cpg = mid / blk.c2.groups; ga.Hin = H1; ga.Win = W1; ga.Ho = Ho; ga.Wo = Wo; ga.stride = r.s3; ga.relu = 1;
      const double fl = 2.0 * (double)B * Ho * Wo * mid * 9.0 * ga.cpg;
      ops.push_back([=](hipStream_t s) { return timed_op(c, "conv_group_kernel", fl, s, [=](hipStream_t st) { return launch_conv_group(dt, ga, st); }); });
      break;
    }
    case Conv2Form::rw3:  // res3 conv2 (3x3, 128 -> 128, stride 1), bf16: weights in registers, LDS holds only the activation halo (conv_rw3.hip)
      RET(add_conv3x3(c, ops, blk.c2, Conv3Route{Conv3Kind::rw3, r.ph, r.pw}, B, H1, W1, r.s3, t1, nullptr, t2, 1));
      break;
    case Conv2Form::generic:
      RET(add_conv3x3(c, ops, blk.c2, Conv3Route{}, B, H1, W1, r.s3, t1, nullptr, t2, 1));
      break;
  }
  if (r.pair_out) return add_res3_pair(c, ops, blk.c3, next->c1, B, Ho * Wo, t2, X, Y, t1);
  if (r.fused_sc) {
    // conv3 + projection shortcut as ONE pointwise GEMM over K = [t2 | X(strided)]: the shortcut
    // tensor is never written to / re-read from HBM
    std::vector<SegDesc> sg = image_segs(B, Ho, Wo, Ho, Wo);
    for (int b = 0; b < B; ++b) { sg[b].in2_row0 = b * Hin * Win; sg[b].in2_W = Win; }
    ConvOpts o3; o3.relu_nch = 1 << 30; o3.in2 = X; o3.in2_ld = Cin; o3.Cin2 = Cin; o3.stride2 = stride;  // (no route depends on stride2)
    RET(add_conv(c, ops, blk.c3sc, t2, mid, Y, cout, sg, o3));
  } else {
    const void* resid = X;
    if (blk.has_sc) {
      ConvOpts os; os.stride = stride; os.route_stride = route_stride;
      RET(add_conv(c, ops, blk.sc, X, Cin, sc, cout, image_segs(B, Hin, Win, Ho, Wo), os));
      resid = sc;
    }
    ConvOpts o3; o3.relu_nch = 1 << 30; o3.res = resid; o3.res_ld = cout; o3.res_mode = 1;
    RET(add_conv(c, ops, blk.c3, t2, mid, Y, cout, image_segs(B, Ho, Wo, Ho, Wo), o3));
  }
  return 0;
}

// One ResNet BasicBlock (detectron2 BasicBlock of R-18 / R-34: 3x3 (stride) -> 3x3, FrozenBN folded, identity or 1x1 projection
// shortcut) appended to `ops`: X [B][Hin*Win][Cin] -> Y [B][Ho*Wo][cout]; scr.t1 (the block's intermediate) and scr.sc (the projected
// shortcut) hold B * Ho * Wo * cout elements.  Shared by build_backbone and the parity entry sylph_basic_block.
//   t = relu(bn1(conv1(x)))        res2: conv_rw64; res3 identity blocks: conv_rw3; else add_conv (pick_conv3_route)
//   sc = x | bn(shortcut(x))       a launch of its own (1x1, stride 2)
//   y = relu(bn2(conv2(t)) + sc)   res2: conv_rw64 with the residual; else add_conv (conv_igemm halo tiles: the only 3x3 route with a residual)
int add_basic_block(sylph_ctx* c, std::vector<OpFn>& ops, const sylph_ctx::Block& blk, int B, const void* X, int Cin, int Hin, int Win,
                    int stride, int cout, void* Y, const BkScratch& scr) {
  const int Ho = (Hin - 1) / stride + 1, Wo = (Win - 1) / stride + 1;
  void *t = scr.t1, *sc = scr.sc;
  if (!blk.has_sc && (Cin != cout || stride != 1)) return fail("internal: BasicBlock without a shortcut must keep its shape");
  if (blk.c1.Cin != Cin || blk.c1.Cout != cout || blk.c2.Cin != cout || blk.c2.Cout != cout || blk.c1.KH != 3 || blk.c2.KH != 3)
    return fail("internal: BasicBlock shape");
  RET(add_conv3x3(c, ops, blk.c1, pick_conv3_route(c, blk.c1, B, Hin, Win, stride), B, Hin, Win, stride, X, nullptr, t, 1));
  const void* resid = X;
  if (blk.has_sc) {
    ConvOpts os; os.stride = stride;
    RET(add_conv(c, ops, blk.sc, X, Cin, sc, cout, image_segs(B, Hin, Win, Ho, Wo), os));
    resid = sc;
  }
  // conv2 adds the shortcut: conv_rw64 takes a residual (the res2 blocks: 64 -> 64, stride 1), conv_rw3 does not
  const bool c64 = Cin == 64 && cout == 64 && stride == 1;
  return add_conv3x3(c, ops, blk.c2, c64 ? pick_conv3_route(c, blk.c2, B, Ho, Wo, 1) : Conv3Route{}, B, Ho, Wo, 1, t, resid, Y, 1);
}

StemRoute pick_stem_route(const sylph_ctx* c) {
  if (c->dt != DT_BF16 || !c->stem_wp || !knob::stem_kernel()) return StemRoute::igemm;
  return knob::fuse_stem_pool() ? StemRoute::fused_pool : StemRoute::stem_conv;
}

// One depthwise 3x3 conv (pad 1) + FrozenBN + ReLU6 on the ReLU6 of its input (conv_dw.hip) appended to `ops`: channels [0, C) of
// x [B][H * W][ld] -> y [B][Ho * Wo][ld]
int add_dwconv3x3(sylph_ctx* c, std::vector<OpFn>& ops, const float* w, const float* scale, const float* shift, int B, int C, int ld, int H, int W,
                  int stride, const void* x, void* y) {
  if (C < 8 || (C & 7) || ld < C || (ld & 7) || (stride != 1 && stride != 2)) return fail("internal: dwconv3x3 needs C % 8 == 0, ld % 8 == 0 and stride 1 or 2");
  DwConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.y = y; a.w = w; a.scale = scale; a.shift = shift;
  a.B = B; a.C = C; a.ld = ld; a.H = H; a.W = W; a.Ho = (H - 1) / stride + 1; a.Wo = (W - 1) / stride + 1; a.stride = stride;
  const double fl = 2.0 * (double)B * a.Ho * a.Wo * C * 9.0;
  const DType dt = c->dt;
  ops.push_back([=](hipStream_t s) { return timed_op(c, "dwconv3x3_kernel", fl, s, [=](hipStream_t st) { return launch_dwconv3x3(dt, a, st); }); });
  return 0;
}

// One MobileNetV2 InvertedResidual block (AdelaiDet mobilenet.py) as a chain of launches:
//   h1 = bn(expand 1x1 (x))                      add_conv, NO activation: the depthwise kernel clamps on load (t == 1: no expand, h1 = x --
//                                                x is then the ReLU6 output of features.0, which the clamp leaves as it is)
//   h2 = relu6(bn(dw 3x3 (relu6(h1))))           conv_dw.hip
//   y  = bn(project 1x1 (h2)) [+ x]              add_conv with the residual input; nothing after the add
// The three bf16 rounding points are h1, h2 and y.
static Mbv2Args mbv2_args(const sylph_ctx::MbBlock& blk, int B, const void* X, int Hin, int Win, void* Y) {
  Mbv2Args a;
  memset(&a, 0, sizeof(a));
  a.x = X; a.y = Y;
  a.w1 = blk.t != 1 ? blk.fw1 : nullptr; a.w2 = blk.fw2;
  a.s1 = blk.exp.scale; a.b1 = blk.exp.shift; a.wd = blk.dw_w; a.sd = blk.dw_scale; a.bd = blk.dw_shift; a.s2 = blk.proj.scale; a.b2 = blk.proj.shift;
  a.B = B; a.H = Hin; a.W = Win; a.Ho = (Hin - 1) / blk.stride + 1; a.Wo = (Win - 1) / blk.stride + 1; a.stride = blk.stride;
  a.cin_p = blk.cin_p; a.cin_ld = blk.cin_ld; a.hid_p = blk.hid_p; a.cout_p = blk.cout_p; a.cout_ld = blk.cout_ld; a.residual = blk.residual();
  return a;
}

// Which launches run one InvertedResidual block.  fp32 and f32s always take the chain.  bf16: SYLPH_MBV2_FUSED 0 = chain, 2 = the
// one-launch kernel wherever it can run, 1 = the block shapes (cin, t, cout, stride) at which it beat the chain in the per-block
// measurement (profiles/mobilenet_layers.txt); every other shape takes the chain.
Mbv2Route pick_mbv2_route(const sylph_ctx* c, const sylph_ctx::MbBlock& blk, int B, int Hin, int Win) {
  const int k = knob::mbv2_fused();
  if (c->dt != DT_BF16 || k <= 0 || !blk.fw2 || (blk.t != 1 && !blk.fw1)) return Mbv2Route::chain;
  if (!conv_mbv2_can_run(mbv2_args(blk, B, blk.fw2, Hin, Win, blk.fw2))) return Mbv2Route::chain;  // (the tensors' addresses play no part)
  if (k >= 2) return Mbv2Route::fused;
  // B = 16 at the 800 x 1344 map sizes, kernel time chain / fused: features.1 0.83 / 0.75 ms, features.3 0.87 / 0.57 ms, features.5-6
  // 0.21 / 0.16 ms; (64, 6, 64, 1) ties (0.10 / 0.10) and every other shape loses (stride 2: 0.79 / 1.64 ms at features.2)
  static const int pays[][4] = {{32, 1, 16, 1}, {24, 6, 24, 1}, {32, 6, 32, 1}};
  for (auto& s : pays)
    if (s[0] == blk.cin && s[1] == blk.t && s[2] == blk.cout && s[3] == blk.stride) return Mbv2Route::fused;
  return Mbv2Route::chain;
}

// Images per run of the chain.  conv_igemm addresses its operands with 31-bit element offsets: a batch whose largest tensor of this block
// passes that is built as several chains over runs of `*run` images and a shorter last one.  One image that passes it alone is refused.
int mbv2_chain_run(const sylph_ctx::MbBlock& blk, int B, int Hin, int Win, int* run) {
  const int Ho = (Hin - 1) / blk.stride + 1, Wo = (Win - 1) / blk.stride + 1;
  const size_t per_img = std::max((size_t)Hin * Win * std::max(blk.cin_ld, blk.t != 1 ? blk.hid_ld : 0), (size_t)Ho * Wo * std::max(blk.hid_ld, blk.cout_ld));
  if (per_img > (size_t)0x7fffffff) return fail("image too large for the MobileNetV2 chain: " + std::to_string(per_img) + " elements per image");
  *run = (int)std::min<size_t>((size_t)B, (size_t)0x7fffffff / per_img);
  return 0;
}

int add_mbv2_block(sylph_ctx* c, std::vector<OpFn>& ops, const sylph_ctx::MbBlock& blk, int B, const void* X, int Hin, int Win, void* Y, void* h1, void* h2) {
  const int Ho = (Hin - 1) / blk.stride + 1, Wo = (Win - 1) / blk.stride + 1;
  if (pick_mbv2_route(c, blk, B, Hin, Win) == Mbv2Route::fused) {
    const Mbv2Args a = mbv2_args(blk, B, X, Hin, Win, Y);
    const double fl = 2.0 * ((double)B * Hin * Win * (blk.t != 1 ? (double)blk.cin * blk.cin * blk.t : 0.0) + (double)B * Ho * Wo * blk.cin * blk.t * (9.0 + blk.cout));
    ops.push_back([=](hipStream_t s) { return timed_op(c, "conv_mbv2_kernel", fl, s, [=](hipStream_t st) { return launch_conv_mbv2(a, st); }); });
    return 0;
  }
  // the runs all go through the same h1 / h2 (the launches of one op list run in order)
  int chunk = 0;
  RET(mbv2_chain_run(blk, B, Hin, Win, &chunk));
  if (chunk < B) {
    const size_t e = c->esz();
    for (int b0 = 0; b0 < B; b0 += chunk)
      RET(add_mbv2_block(c, ops, blk, std::min(chunk, B - b0), (const char*)X + (size_t)b0 * Hin * Win * blk.cin_ld * e, Hin, Win,
                         (char*)Y + (size_t)b0 * Ho * Wo * blk.cout_ld * e, h1, h2));
    return 0;
  }
  const void* dw_in = X;
  if (blk.t != 1) {
    RET(add_conv(c, ops, blk.exp, X, blk.cin_ld, h1, blk.hid_ld, image_segs(B, Hin, Win, Hin, Win), ConvOpts()));
    dw_in = h1;
  }
  // (t == 1: hidden = input, read at the input's pitch and written at the same one: cin_ld == hid_ld)
  RET(add_dwconv3x3(c, ops, blk.dw_w, blk.dw_scale, blk.dw_shift, B, blk.hid_p, blk.hid_ld, Hin, Win, blk.stride, dw_in, h2));
  ConvOpts o3;
  if (blk.residual()) { o3.res = X; o3.res_ld = blk.cin_ld; o3.res_mode = 1; }
  return add_conv(c, ops, blk.proj, h2, blk.hid_ld, Y, blk.cout_ld, image_segs(B, Ho, Wo, Ho, Wo), o3);
}

// What a bottom-up path hands to the FPN: res2..res5 as dense images [B][h * w][ld], c logical channels
struct Trunk {
  const void* out[4] = {nullptr, nullptr, nullptr, nullptr};
  int h[4] = {0, 0, 0, 0}, w[4] = {0, 0, 0, 0}, c[4] = {0, 0, 0, 0}, ld[4] = {0, 0, 0, 0};
};

// MobileNetV2 bottom-up (cfg.mobilenet): features.0 on the normalised batch, then the 17 blocks.  res2..res5 (features 3 / 6 / 13 / 17) get
// buffers of their own (the parity taps and the laterals read them after the step); every other block output goes to two ping-pong buffers.
static int build_mbv2_trunk(sylph_ctx* c, Plan* P, Trunk* T) {
  const int B = P->B, H = P->H, W = P->W;
  const size_t e = c->esz();
  if (c->mb_blocks.size() != 17 || !c->mb_stem_w) return fail("internal: MobileNetV2 weights");
  RET(c->dalloc(&P->x0, (size_t)B * H * W * 4 * e));
  RET(c->dalloc((void**)&P->img_desc_dev, sizeof(ImageDesc) * B));
  HIPCHK(hipHostMalloc((void**)&P->img_desc_host, sizeof(ImageDesc) * B));
  auto& ops = P->backbone_ops;
  int Hin = (H - 1) / 2 + 1, Win = (W - 1) / 2 + 1;
  // sizes of the shared buffers: the largest block output that is not a stage output, the largest expand / depthwise outputs
  size_t n_y = 0, n_h1 = 0, n_h2 = 0;
  {
    int h = Hin, w = Win;
    for (size_t i = 0; i < c->mb_blocks.size(); ++i) {
      const auto& blk = c->mb_blocks[i];
      const int ho = (h - 1) / blk.stride + 1, wo = (w - 1) / blk.stride + 1;
      if (blk.t != 1) n_h1 = std::max(n_h1, (size_t)B * h * w * blk.hid_ld);
      n_h2 = std::max(n_h2, (size_t)B * ho * wo * blk.hid_ld);
      n_y = std::max(n_y, (size_t)B * ho * wo * blk.cout_ld);
      h = ho; w = wo;
    }
  }
  const int c0 = c->mb_blocks[0].cin_p, ld0 = c->mb_blocks[0].cin_ld;
  void *s0, *Ya, *Yb, *h1, *h2;
  RET(c->dalloc(&s0, (size_t)B * Hin * Win * ld0 * e));
  RET(c->dalloc(&Ya, n_y * e));
  RET(c->dalloc(&Yb, n_y * e));
  RET(c->dalloc(&h1, n_h1 * e));
  RET(c->dalloc(&h2, n_h2 * e));
  {
    MbStemArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.x = P->x0; sa.y = s0; sa.w = c->mb_stem_w; sa.scale = c->mb_stem_scale; sa.shift = c->mb_stem_shift;
    sa.B = B; sa.C = c0; sa.ld = ld0; sa.H = H; sa.W = W; sa.Ho = Hin; sa.Wo = Win;
    const double fl = 2.0 * (double)B * Hin * Win * 32.0 * 27.0;
    const DType dt = c->dt;
    ops.push_back([=](hipStream_t s) { return timed_op(c, "mbv2_stem_kernel", fl, s, [=](hipStream_t st) { return launch_mbv2_stem(dt, sa, st); }); });
  }
  P->stem_takes_raw = false;  // sylph_preprocess writes x0
  const void* X = s0;
  void* Y = nullptr;
  for (size_t i = 0; i < c->mb_blocks.size(); ++i) {
    const auto& blk = c->mb_blocks[i];
    const int Ho = (Hin - 1) / blk.stride + 1, Wo = (Win - 1) / blk.stride + 1;
    const int si = i == 2 ? 0 : i == 5 ? 1 : i == 12 ? 2 : i == 16 ? 3 : -1;  // features 3 / 6 / 13 / 17
    void* dst;
    if (si >= 0) RET(c->dalloc(&dst, (size_t)B * Ho * Wo * blk.cout_ld * e));
    else dst = Y = (Y == Ya) ? Yb : Ya;
    RET(add_mbv2_block(c, ops, blk, B, X, Hin, Win, dst, h1, h2));
    X = dst; Hin = Ho; Win = Wo;
    if (si >= 0) { T->out[si] = dst; T->h[si] = Ho; T->w[si] = Wo; T->c[si] = blk.cout; T->ld[si] = blk.cout_ld; }
  }
  for (int si = 0; si < 4; ++si) {
    P->stage_out[si] = T->out[si]; P->stage_h[si] = T->h[si]; P->stage_w[si] = T->w[si]; P->stage_c[si] = T->c[si]; P->stage_ld[si] = T->ld[si];
  }
  return 0;
}

static int build_resnet_trunk(sylph_ctx* c, Plan* P, Trunk* T) {
  const int B = P->B, H = P->H, W = P->W;
  const size_t e = c->esz();
  RET(c->dalloc(&P->x0, (size_t)B * H * W * 4 * e));
  const int H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1;
  const int H4 = (H2 - 1) / 2 + 1, W4 = (W2 - 1) / 2 + 1;
  RET(c->dalloc(&P->stem_out, (size_t)B * H2 * W2 * 64 * e));
  RET(c->dalloc(&P->pool_out, (size_t)B * H4 * W4 * 64 * e));
  RET(c->dalloc((void**)&P->img_desc_dev, sizeof(ImageDesc) * B));
  HIPCHK(hipHostMalloc((void**)&P->img_desc_host, sizeof(ImageDesc) * B));
  auto& ops = P->backbone_ops;
  const DType dt = c->dt;
  {
    void *so = P->stem_out, *po = P->pool_out;
    ConvOpts os; os.stem = 1; os.relu_nch = 1 << 30;
    os.flops = 2.0 * (double)B * H2 * W2 * 64.0 * 147.0;
    const void *x0 = P->x0, *wp = c->stem_wp;
    const float *scl = c->stem.scale, *shf = c->stem.shift;
    const double fl = os.flops;
    switch (pick_stem_route(c)) {
      case StemRoute::fused_pool: {  // stem + max-pool in one kernel: the 64-channel stem output never reaches HBM (stem_conv.hip)
        void* trash = nullptr;
        RET(c->dalloc(&trash, (size_t)512 * 256 * 16));
        const Plan* PP = P;
        ops.push_back([=](hipStream_t s) {
          return timed_op(c, "stem_pool_kernel", fl, s, [=](hipStream_t st) {
            if (PP->raw_input)  // (p - mean) / std applied on the way into the stem's LDS patch: no normalised copy of the batch
              return launch_stem_pool_raw(PP->img_desc_dev, c->cfg.pixel_mean, c->cfg.pixel_std, wp, scl, shf, po, trash, B, H, W, H2, W2, H4, W4, st);
            return launch_stem_pool(x0, wp, scl, shf, po, trash, B, H, W, H2, W2, H4, W4, st);
          });
        });
        P->stem_takes_raw = B <= STEM_RAW_MAX_BATCH;
        break;
      }
      case StemRoute::stem_conv:
        ops.push_back([=](hipStream_t s) {
          return timed_op(c, "stem_conv_kernel", fl, s, [=](hipStream_t st) { return launch_stem_conv(x0, wp, scl, shf, so, B, H, W, H2, W2, st); });
        });
        ops.push_back([=](hipStream_t s) { return launch_maxpool(dt, so, po, B, H2, W2, 64, H4, W4, s); });
        break;
      case StemRoute::igemm:
        RET(add_conv(c, ops, c->stem, P->x0, 4, so, 64, image_segs(B, H, W, H2, W2), os));
        ops.push_back([=](hipStream_t s) { return launch_maxpool(dt, so, po, B, H2, W2, 64, H4, W4, s); });
        break;
    }
  }
  const void* X = P->pool_out;
  int Hin = H4, Win = W4, Cin = 64;
  const void* stage_out[4] = {nullptr, nullptr, nullptr, nullptr};
  int stage_h[4], stage_w[4];
  const bool basic = !c->stages[0].empty() && c->stages[0][0].basic;  // R-18 / R-34: BasicBlocks, stage widths 64 << si
  int stage_c[4];
  // The last block of a stage that no one reads but the next stage's strided 1x1 convs (res2 with STRIDE_IN_1X1: res3.0's conv1 and
  // shortcut take every other row and column, and res2 is no FPN input) computes only those positions, into a compact tensor (bottleneck.hip,
  // EVEN): a quarter of its conv2 / conv3 work and of its stores.  The next block then runs its own launches on that tensor with stride 1.
  // SYLPH_BK_STRIDED_TAIL: 0 off, 1 (default) on.
  bool in_compact = false;  // X is such a compact tensor (Hin x Win its size)
  for (int si = 0; si < 4; ++si) {
    const int mid = (c->cfg.num_groups * c->cfg.width_per_group) << si, cout = (basic ? 64 : 256) << si;  // (ResNeXt: num_groups > 1)
    const int first_stride = si == 0 ? 1 : in_compact ? 1 : 2;
    const int Hs = (Hin - 1) / first_stride + 1, Ws = (Win - 1) / first_stride + 1;
    void *t1, *t2 = nullptr, *sc, *Ya, *Yb;
    // t1 may still be at the input resolution when the stride sits on the 3x3 (a BasicBlock's one intermediate is at the output's)
    RET(c->dalloc(&t1, basic ? (size_t)B * Hs * Ws * cout * e : (size_t)B * Hin * Win * mid * e));
    if (!basic) RET(c->dalloc(&t2, (size_t)B * Hs * Ws * mid * e));
    RET(c->dalloc(&sc, (size_t)B * Hs * Ws * cout * e));
    RET(c->dalloc(&Ya, (size_t)B * Hs * Ws * cout * e));
    RET(c->dalloc(&Yb, (size_t)B * Hs * Ws * cout * e));
    auto& blocks = c->stages[si];
    void* Y = nullptr;
    BkScratch scr{t1, t2, sc, &P->bk_trash};
    bool pair_in = false;  // the block before computed this block's conv1
    for (size_t bi = 0; bi < blocks.size(); ++bi) {
      const int stride = bi == 0 ? first_stride : 1;
      Y = (Y == Ya) ? Yb : Ya;
      const bool fpn_input = si >= 1;
      const bool even_tail = knob::bk_strided_tail() && !basic && bi > 0 && bi + 1 == blocks.size() && !fpn_input && si + 1 < 4 && c->cfg.stride_in_1x1 &&
                             !c->stages[si + 1].empty() && !c->stages[si + 1][0].basic &&
                             pick_block_route(c, blocks[bi], B, Cin, Hin, Win, stride, mid, cout, 0).tail_ok;
      // res3 identity blocks (SYLPH_BLOCK_PAIR): block bi's conv3 launch also computes block bi + 1's conv1, which is then not built
      const sylph_ctx::Block* nextb = !basic && bi + 1 < blocks.size() ? &blocks[bi + 1] : nullptr;
      const bool pair_out = nextb && pick_block_route(c, blocks[bi], B, Cin, Hin, Win, stride, mid, cout, 0, nextb).pair_ok;
      if (basic) RET(add_basic_block(c, ops, blocks[bi], B, X, Cin, Hin, Win, stride, cout, Y, scr));
      else RET(add_bottleneck(c, ops, blocks[bi], B, X, Cin, Hin, Win, stride, mid, cout, Y, scr,
                              (even_tail ? BK_EVEN_OUT : (bi == 0 && in_compact) ? BK_IN_COMPACT : 0) | (pair_out ? BK_PAIR_OUT : 0) | (pair_in ? BK_PAIR_IN : 0),
                              nextb));
      pair_in = pair_out;
      if (bi == 0) in_compact = false;
      if (even_tail) {  // the dense output exists on demand only (sylph_export_stage)
        P->tail_even = true; P->tail_x = X;
        P->stage_h[si] = Hin; P->stage_w[si] = Win; P->stage_c[si] = cout;
        in_compact = true;
        X = Y; Hin /= 2; Win /= 2; Cin = cout;
        continue;
      }
      X = Y; Hin = (Hin - 1) / stride + 1; Win = (Win - 1) / stride + 1; Cin = cout;
    }
    stage_out[si] = X; stage_h[si] = Hin; stage_w[si] = Win; stage_c[si] = cout;
    if (in_compact) continue;  // (P->stage_h / _w / _c hold the dense shape; P->stage_out[si] stays empty)
    P->stage_out[si] = X; P->stage_h[si] = Hin; P->stage_w[si] = Win; P->stage_c[si] = cout;
  }
  for (int si = 0; si < 4; ++si) { T->out[si] = stage_out[si]; T->h[si] = stage_h[si]; T->w[si] = stage_w[si]; T->c[si] = T->ld[si] = stage_c[si]; }
  return 0;
}

int build_backbone(sylph_ctx* c, Plan* P) {
  if (P->backbone_built) return 0;
  if (!c->has_backbone) return fail("backbone weights were not loaded");
  const int B = P->B;
  const size_t e = c->esz();
  RET(ensure_pyramid(c, P));
  Trunk T;
  if (c->cfg.mobilenet) RET(build_mbv2_trunk(c, P, &T));
  else RET(build_resnet_trunk(c, P, &T));
  auto& ops = P->backbone_ops;
  const DType dt = c->dt;
  const void* const* stage_out = T.out;
  const int *stage_h = T.h, *stage_w = T.w, *stage_ld = T.ld;
  // FPN (res3..res5 -> p3..p5), top-down with nearest 2x upsample fused as a residual, then P6/P7
  // Small batches: after lateral5 the FPN is two independent chains of small launches -- {output5, P6, relu, P7} and {lateral4, output4,
  // lateral3, output3} -- so the first one runs on the context's side stream between a fork and a join (as the bbox tower does,
  // api_head.hip); large batches keep one stream.
  const int fpn_two_on = knob::head_streams();
  const bool fpn_two = fpn_two_on == 2 || (fpn_two_on == 1 && (size_t)B * P->Ltot <= (size_t)32 * 22400);  // (round 6: 32 images, as the head)
  if (fpn_two) RET(ensure_side_stream(c));
  std::vector<OpFn> side_ops;
  void* lat[3] = {nullptr, nullptr, nullptr};
  for (int k = 2; k >= 0; --k) {
    const int si = k + 1, h = stage_h[si], w = stage_w[si], cin = stage_ld[si];
    if (h != P->hl[k] || w != P->wl[k]) return fail("internal: level geometry mismatch");
    RET(c->dalloc(&lat[k], (size_t)B * h * w * 256 * e));
    ConvOpts ol;
    std::vector<SegDesc> segs = image_segs(B, h, w, h, w);
    if (k < 2) {
      ol.res = lat[k + 1]; ol.res_ld = 256; ol.res_mode = 2;
      segs = image_segs(B, h, w, h, w, stage_h[si + 1], stage_w[si + 1]);
      if (h != 2 * stage_h[si + 1] || w != 2 * stage_w[si + 1]) return fail("FPN needs exact 2x level sizes");
    }
    RET(add_conv(c, ops, c->fpn_lat[k], stage_out[si], cin, lat[k], 256, segs, ol));
    if (k == 2 && fpn_two) ops.push_back(side_fork_op(c));  // right behind lateral5: the side stream continues from here
    std::vector<SegDesc> so = image_segs(B, h, w, h, w);
    for (int b = 0; b < B; ++b) so[b].out_row0 = b * P->Ltot + P->off[k];
    ConvOpts oo; oo.pad = 1; oo.stream_slot = (k == 2 && fpn_two) ? 1 : 0;
    RET(add_conv(c, (k == 2 && fpn_two) ? side_ops : ops, c->fpn_out[k], lat[k], 256, P->F, 256, so, oo));
  }
  std::vector<OpFn>& top_ops = fpn_two ? side_ops : ops;  // P6 / P7 hang off output5
  for (int k = 3; k < c->cfg.nlevels && k < 5; ++k) {
    std::vector<SegDesc> sg = image_segs(B, P->hl[k - 1], P->wl[k - 1], P->hl[k], P->wl[k]);
    for (int b = 0; b < B; ++b) {
      sg[b].in_row0 = b * P->Ltot + P->off[k - 1];
      sg[b].out_row0 = b * P->Ltot + P->off[k];
    }
    ConvOpts op; op.stride = 2; op.pad = 1; op.stream_slot = fpn_two ? 1 : 0;
    const void* src = P->F;
    if (k == 4) {  // P7 = conv(relu(P6)): rectified copy of the P6 rows
      const int n6 = P->hl[3] * P->wl[3];
      void* p6r;
      RET(c->dalloc(&p6r, (size_t)B * n6 * 256 * e));
      std::vector<CopySeg> cs;
      for (int b = 0; b < B; ++b) {
        cs.push_back(CopySeg{b * P->Ltot + P->off[3], b * n6, n6});
        sg[b].in_row0 = b * n6;
      }
      CopySeg* csd;
      RET(upload(c, (void**)&csd, cs.data(), cs.size() * sizeof(CopySeg)));
      const void* F = P->F;
      top_ops.push_back([=](hipStream_t s) { return launch_relu_rows(dt, F, p6r, 256, csd, B, n6, s); });
      src = p6r;
    }
    RET(add_conv(c, top_ops, k == 3 ? c->p6 : c->p7, src, 256, P->F, 256, sg, op));
  }
  if (fpn_two) {
    for (const OpFn& op : side_ops) ops.push_back(on_side_stream(c, op));
    ops.push_back(side_join_op(c));
  }
  P->backbone_built = true;
  return 0;
}

}  // namespace sylph_host

extern "C" {

int sylph_preprocess(sylph_ctx* c, int B, const float* const* images, const int* hs, const int* ws, int* ph, int* pw) {
  if (!c->finalized) return fail("weights not finalized");
  if (B <= 0) return fail("empty batch");
  HIPCHK(hipSetDevice(c->device));
  int mh = 0, mw = 0;
  for (int b = 0; b < B; ++b) { mh = hs[b] > mh ? hs[b] : mh; mw = ws[b] > mw ? ws[b] : mw; }
  const int d = c->cfg.size_divisibility;
  if (d > 1) { mh = (mh + d - 1) / d * d; mw = (mw + d - 1) / d * d; }
  Plan* P = get_plan(c, B, mh, mw);
  OwnerScope own(c, P);
  BUILD(build_backbone(c, P), P);
  // image table of this call; the H2D copy is skipped when the device table already holds it (a caller that reuses its input buffers:
  // every step of a steady query stream).  Otherwise the previous batch's H2D copy of the pinned table must have been consumed: wait for
  // THAT copy only (an event), not for the stream: the host stays free to enqueue the next step behind the running one
  std::vector<ImageDesc> tab((size_t)B);
  for (int b = 0; b < B; ++b) {
    tab[b].ptr = images[b]; tab[b].h = hs[b]; tab[b].w = ws[b];
    P->img_h[b] = hs[b]; P->img_w[b] = ws[b];
  }
  if (!P->img_desc_ev || P->img_desc_kind != 1 || P->img_desc_last.size() != tab.size() ||
      memcmp(P->img_desc_last.data(), tab.data(), tab.size() * sizeof(ImageDesc)) != 0) {
    if (P->img_desc_ev) HIPCHK(hipEventSynchronize(P->img_desc_ev));
    else HIPCHK(hipEventCreateWithFlags(&P->img_desc_ev, hipEventDisableTiming));
    memcpy(P->img_desc_host, tab.data(), tab.size() * sizeof(ImageDesc));
    HIPCHK(hipMemcpyAsync(P->img_desc_dev, P->img_desc_host, sizeof(ImageDesc) * B, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(P->img_desc_ev, c->stream));
    P->img_desc_last = tab;
    P->img_desc_kind = 1;
  }
  P->raw_input = knob::fuse_preprocess() && P->stem_takes_raw;  // read per call (tests compare the two paths in one process)
  if (!P->raw_input)
    KCHK(launch_preprocess(c->dt, P->img_desc_dev, P->x0, B, mh, mw, c->cfg.pixel_mean, c->cfg.pixel_std, c->stream),
         "preprocess");
  begin_fresh_batch(c, P);
  c->cur = P;
  if (ph) *ph = mh;
  if (pw) *pw = mw;
  return 0;
}

int sylph_preprocess_u8(sylph_ctx* c, int B, const unsigned char* const* images, const int* hs, const int* ws, const int* nhs,
                        const int* nws, int rgb_input, int* ph, int* pw) {
  if (!c->finalized) return fail("weights not finalized");
  if (B <= 0) return fail("empty batch");
  HIPCHK(hipSetDevice(c->device));
  int mh = 0, mw = 0;
  for (int b = 0; b < B; ++b) {
    if (hs[b] <= 0 || ws[b] <= 0 || nhs[b] <= 0 || nws[b] <= 0) return fail("sylph_preprocess_u8: bad image size");
    mh = nhs[b] > mh ? nhs[b] : mh; mw = nws[b] > mw ? nws[b] : mw;
  }
  const int d = c->cfg.size_divisibility;
  if (d > 1) { mh = (mh + d - 1) / d * d; mw = (mw + d - 1) / d * d; }
  Plan* P = get_plan(c, B, mh, mw);
  OwnerScope own(c, P);
  BUILD(build_backbone(c, P), P);
  // resampling tables of every image (cached per (in, out) size pair), laid out back to back
  std::vector<std::shared_ptr<PilCoeffs>> hc((size_t)B), vc((size_t)B);
  size_t nint = 0;
  for (int b = 0; b < B; ++b) {
    for (int pass = 0; pass < 2; ++pass) {
      const std::pair<int, int> key = pass == 0 ? std::make_pair(ws[b], nws[b]) : std::make_pair(hs[b], nhs[b]);
      auto it = c->pil_cache.find(key);
      if (it == c->pil_cache.end()) {
        if (c->pil_cache.size() > 256) c->pil_cache.clear();
        it = c->pil_cache.emplace(key, pil_bilinear_coeffs(key.first, key.second)).first;
      }
      (pass == 0 ? hc : vc)[b] = it->second;
      nint += it->second->bounds.size() + it->second->kk.size();
    }
  }
  if (P->img_desc_ev) HIPCHK(hipEventSynchronize(P->img_desc_ev));
  else HIPCHK(hipEventCreateWithFlags(&P->img_desc_ev, hipEventDisableTiming));
  const size_t need = sizeof(ResizeDesc) * B + nint * sizeof(int);
  if (need > P->rz_tab_cap) {
    if (P->rz_host) (void)hipHostFree(P->rz_host);
    if (P->rz_desc_dev) c->dfree(P->rz_desc_dev);
    P->rz_host = nullptr; P->rz_desc_dev = nullptr; P->rz_tab_cap = 0;
    const size_t cap = need + need / 2;
    HIPCHK(hipHostMalloc((void**)&P->rz_host, cap));
    RET(c->dalloc((void**)&P->rz_desc_dev, cap));
    P->rz_tab_cap = cap;
  }
  ResizeDesc* dh = reinterpret_cast<ResizeDesc*>(P->rz_host);
  int* th = reinterpret_cast<int*>(P->rz_host + sizeof(ResizeDesc) * B);
  size_t off = 0;
  for (int b = 0; b < B; ++b) {
    ResizeDesc& r = dh[b];
    r.src = images[b]; r.h = hs[b]; r.w = ws[b]; r.new_h = nhs[b]; r.new_w = nws[b];
    r.ksh = hc[b]->ksize; r.ksv = vc[b]->ksize;
    r.hb_off = (int)off; memcpy(th + off, hc[b]->bounds.data(), hc[b]->bounds.size() * sizeof(int)); off += hc[b]->bounds.size();
    r.hk_off = (int)off; memcpy(th + off, hc[b]->kk.data(), hc[b]->kk.size() * sizeof(int)); off += hc[b]->kk.size();
    r.vb_off = (int)off; memcpy(th + off, vc[b]->bounds.data(), vc[b]->bounds.size() * sizeof(int)); off += vc[b]->bounds.size();
    r.vk_off = (int)off; memcpy(th + off, vc[b]->kk.data(), vc[b]->kk.size() * sizeof(int)); off += vc[b]->kk.size();
    P->img_h[b] = nhs[b]; P->img_w[b] = nws[b];
  }
  HIPCHK(hipMemcpyAsync(P->rz_desc_dev, P->rz_host, need, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(P->img_desc_ev, c->stream));
  const int* tab_dev = reinterpret_cast<const int*>(reinterpret_cast<const char*>(P->rz_desc_dev) + sizeof(ResizeDesc) * B);
  P->raw_input = false;  // this pipeline writes the normalised batch itself
  KCHK(launch_resize_preprocess(c->dt, P->rz_desc_dev, tab_dev, P->x0, B, mh, mw, c->cfg.pixel_mean, c->cfg.pixel_std, rgb_input,
                                c->stream), "resize_preprocess");
  begin_fresh_batch(c, P);
  c->cur = P;
  if (ph) *ph = mh;
  if (pw) *pw = mw;
  return 0;
}

/* see include/sylph_hip.h */
int sylph_preprocess_views(sylph_ctx* c, int B, const unsigned char* const* src, const int* shs, const int* sws, const int* cx0, const int* cy0,
                           const int* cws, const int* chs, const int* nhs, const int* nws, const int* flip, int rgb_input, int* ph, int* pw) {
  if (!c->finalized) return fail("weights not finalized");
  if (B <= 0) return fail("empty batch");
  if (!src || !shs || !sws || !cx0 || !cy0 || !cws || !chs || !nhs || !nws || !flip) return fail("sylph_preprocess_views: NULL argument");
  int mh = 0, mw = 0;
  for (int b = 0; b < B; ++b) {
    if (!src[b]) return fail("sylph_preprocess_views: view " + std::to_string(b) + " has no source");
    if (shs[b] <= 0 || sws[b] <= 0 || cws[b] <= 0 || chs[b] <= 0 || nhs[b] <= 0 || nws[b] <= 0)
      return fail("sylph_preprocess_views: view " + std::to_string(b) + " has a non-positive size");
    if (cx0[b] < 0 || cy0[b] < 0 || cws[b] > sws[b] - cx0[b] || chs[b] > shs[b] - cy0[b])
      return fail("sylph_preprocess_views: view " + std::to_string(b) + ": crop (" + std::to_string(cx0[b]) + ", " + std::to_string(cy0[b]) + ") + " +
                  std::to_string(cws[b]) + " x " + std::to_string(chs[b]) + " leaves its " + std::to_string(sws[b]) + " x " + std::to_string(shs[b]) +
                  " source");
    mh = nhs[b] > mh ? nhs[b] : mh; mw = nws[b] > mw ? nws[b] : mw;
  }
  HIPCHK(hipSetDevice(c->device));
  const int d = c->cfg.size_divisibility;
  if (d > 1) { mh = (mh + d - 1) / d * d; mw = (mw + d - 1) / d * d; }
  Plan* P = get_plan(c, B, mh, mw);
  OwnerScope own(c, P);
  BUILD(build_backbone(c, P), P);
  // resampling tables (cached per (in, out) size pair); the views of one step mostly share a few: each distinct table is laid out once
  std::vector<std::shared_ptr<PilCoeffs>> hc((size_t)B), vc((size_t)B);
  std::map<const PilCoeffs*, size_t> tab_off;
  std::vector<const PilCoeffs*> order;
  size_t nint = 0;
  for (int b = 0; b < B; ++b) {
    for (int pass = 0; pass < 2; ++pass) {
      const std::pair<int, int> key = pass == 0 ? std::make_pair(cws[b], nws[b]) : std::make_pair(chs[b], nhs[b]);
      auto it = c->pil_cache.find(key);
      if (it == c->pil_cache.end()) {
        if (c->pil_cache.size() > 256) { c->pil_cache.clear(); }  // (hc / vc keep this call's tables alive)
        it = c->pil_cache.emplace(key, pil_bilinear_coeffs(key.first, key.second)).first;
      }
      (pass == 0 ? hc : vc)[b] = it->second;
      if (tab_off.emplace(it->second.get(), nint).second) {
        order.push_back(it->second.get());
        nint += it->second->bounds.size() + it->second->kk.size();
      }
    }
  }
  if (nint > (size_t)INT32_MAX) return fail("sylph_preprocess_views: resampling tables too large");
  if (P->img_desc_ev) HIPCHK(hipEventSynchronize(P->img_desc_ev));
  else HIPCHK(hipEventCreateWithFlags(&P->img_desc_ev, hipEventDisableTiming));
  const size_t need = sizeof(ViewDesc) * B + nint * sizeof(int);
  if (need > P->rz_tab_cap) {
    if (P->rz_host) (void)hipHostFree(P->rz_host);
    if (P->rz_desc_dev) c->dfree(P->rz_desc_dev);
    P->rz_host = nullptr; P->rz_desc_dev = nullptr; P->rz_tab_cap = 0;
    const size_t cap = need + need / 2;
    HIPCHK(hipHostMalloc((void**)&P->rz_host, cap));
    RET(c->dalloc((void**)&P->rz_desc_dev, cap));
    P->rz_tab_cap = cap;
  }
  ViewDesc* dh = reinterpret_cast<ViewDesc*>(P->rz_host);
  int* th = reinterpret_cast<int*>(P->rz_host + sizeof(ViewDesc) * B);
  for (const PilCoeffs* pc : order) {
    const size_t off = tab_off[pc];
    memcpy(th + off, pc->bounds.data(), pc->bounds.size() * sizeof(int));
    memcpy(th + off + pc->bounds.size(), pc->kk.data(), pc->kk.size() * sizeof(int));
  }
  for (int b = 0; b < B; ++b) {
    ViewDesc& r = dh[b];
    r.src = src[b]; r.pitch = sws[b]; r.x0 = cx0[b]; r.y0 = cy0[b]; r.new_h = nhs[b]; r.new_w = nws[b]; r.flip = flip[b] ? 1 : 0;
    r.ksh = hc[b]->ksize; r.ksv = vc[b]->ksize;
    r.hb_off = (int)tab_off[hc[b].get()]; r.hk_off = r.hb_off + (int)hc[b]->bounds.size();
    r.vb_off = (int)tab_off[vc[b].get()]; r.vk_off = r.vb_off + (int)vc[b]->bounds.size();
    P->img_h[b] = nhs[b]; P->img_w[b] = nws[b];
  }
  HIPCHK(hipMemcpyAsync(P->rz_desc_dev, P->rz_host, need, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(P->img_desc_ev, c->stream));
  const ViewDesc* desc_dev = reinterpret_cast<const ViewDesc*>(P->rz_desc_dev);
  const int* tab_dev = reinterpret_cast<const int*>(reinterpret_cast<const char*>(P->rz_desc_dev) + sizeof(ViewDesc) * B);
  P->raw_input = false;  // this pipeline writes the normalised batch itself
  void* x0 = P->x0;
  const DType dt = c->dt;
  const float* mean = c->cfg.pixel_mean;
  const float* stdv = c->cfg.pixel_std;
  KCHK(timed_op(c, "view_preprocess_kernel", 0.0, c->stream, [=](hipStream_t st) {
         return launch_view_preprocess(dt, desc_dev, tab_dev, x0, B, mh, mw, mean, stdv, rgb_input, st);
       }), "view_preprocess");
  begin_fresh_batch(c, P);
  c->cur = P;
  if (ph) *ph = mh;
  if (pw) *pw = mw;
  return 0;
}

int sylph_export_input(sylph_ctx* c, float* out) {
  RET(refuse_on_record(c, "sylph_export_input"));
  Plan* P = c->cur;
  if (!P || !P->x0) return fail("sylph_preprocess must be called first");
  if (P->raw_input)  // the normalisation is fused into the stem kernel: x0 has not been written for this batch (raw_input stays set)
    KCHK(launch_preprocess(c->dt, P->img_desc_dev, P->x0, P->B, P->H, P->W, c->cfg.pixel_mean, c->cfg.pixel_std, c->stream), "preprocess");
  KCHK(launch_export_input(c->dt, P->x0, out, P->B, P->H, P->W, c->stream), "export_input");
  return 0;
}

int sylph_backbone_fpn(sylph_ctx* c) {
  RET(refuse_on_record(c, "sylph_backbone_fpn"));
  if (!c->cur || !c->cur->backbone_built) return fail("sylph_preprocess must be called first");
  return run_ops(c, c->cur->backbone_ops, "backbone_fpn");
}

int sylph_import_pyramid(sylph_ctx* c, int B, int H, int W, const int* hs, const int* ws, const float* const* levels) {
  if (!c->finalized) return fail("weights not finalized");
  HIPCHK(hipSetDevice(c->device));
  Plan* P = get_plan(c, B, H, W);
  OwnerScope own(c, P);
  BUILD(ensure_pyramid(c, P), P);
  for (int b = 0; b < B; ++b) { P->img_h[b] = hs ? hs[b] : H; P->img_w[b] = ws ? ws[b] : W; }
  for (int l = 0; l < c->cfg.nlevels; ++l) {
    const int hw = P->hl[l] * P->wl[l];
    for (int b = 0; b < B; ++b)
      KCHK(launch_import_nchw(c->dt, levels[l] + (size_t)b * 256 * hw, P->F, 256, hw, b * P->Ltot + P->off[l], 256,
                              c->stream),
           "import_pyramid");
  }
  begin_fresh_batch(c, P);
  c->cur = P;
  return 0;
}

int sylph_export_pyramid(sylph_ctx* c, int level, float* out) {
  RET(refuse_on_record(c, "sylph_export_pyramid"));
  Plan* P = c->cur;
  if (!P || !P->F) return fail("no current batch");
  if (level < 0 || level >= c->cfg.nlevels) return fail("bad level");
  const int hw = P->hl[level] * P->wl[level];
  for (int b = 0; b < P->B; ++b)
    KCHK(launch_export_nchw(c->dt, P->F, out + (size_t)b * 256 * hw, 256, hw, b * P->Ltot + P->off[level], 256,
                            c->stream),
         "export_pyramid");
  return 0;
}

}  // extern "C"
