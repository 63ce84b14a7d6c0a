// Host side of libsylph_hip.so, unit "views": the merges of the detections of several views of one source (sylph_merge_views,
// sylph_merge_views_large, sylph_stitch_views and the two _bytes entries): argument checks, the view tables, the launches.
// No torch types, no CPU compute fallback: the merges are the HIP kernels of merge_views.hip and merge_views_large.hip.
#include "api_internal.h"

extern "C" {

// The checks both view merges share, `who` named in every message -> per_src: the views of every source
static int merge_check_views(const std::string& who, int n_src, int n_views, const int* view_src, const float* view_x0, const float* view_y0,
                             const float* view_w, const int* view_flip, int max_in, int max_out, bool buffers, std::vector<int>* per_src) {
  if (n_src <= 0) return fail(who + ": no sources (n_src <= 0)");
  if (n_views <= 0) return fail(who + ": no views (n_views <= 0)");
  if (max_in <= 0 || max_out <= 0) return fail(who + ": max_in and max_out must be positive");
  if (!view_src || !view_x0 || !view_y0 || !view_w || !view_flip) return fail(who + ": a view table is NULL");
  if (!buffers) return fail(who + ": a device buffer is NULL");
  if ((long)n_views * max_in >= (1L << 31)) return fail(who + ": n_views * max_in does not fit a row index");
  per_src->assign((size_t)n_src, 0);
  for (int v = 0; v < n_views; ++v) {
    if (view_src[v] < 0 || view_src[v] >= n_src)
      return fail(who + ": view_src[" + std::to_string(v) + "] = " + std::to_string(view_src[v]) + " is outside the " + std::to_string(n_src) + " sources");
    ++(*per_src)[view_src[v]];
  }
  return 0;
}

// The refusal of the two _bytes entries (`who`), else the layout's size
static int64_t merge_workspace_bytes(const std::string& who, const MergeLargeLayout& L, int n_src, int n_views, int max_in) {
  if (L.bytes < 0) {
    fail(who + ": n_src, n_views and max_in must be positive and n_views * max_in must fit a row index (got " + std::to_string(n_src) + ", " +
         std::to_string(n_views) + ", " + std::to_string(max_in) + ")");
    return -1;
  }
  return (int64_t)L.bytes;
}

// The checks the two workspace-taking entries add, `who` named in every message: topk, ...
static int merge_check_topk(const std::string& who, int topk) {
  if (topk < -1) return fail(who + ": topk " + std::to_string(topk) + " (a count, 0 = every kept box, -1 = POST_NMS_TOPK_TEST)");
  return 0;
}

// ... and the rows of every source against MERGE_LARGE_POOL_CAP, then the workspace against L, the entry's layout (which cannot refuse any
// more after merge_check_views); who + "_bytes" is the entry that gives its size
static int merge_check_workspace(const std::string& who, const std::vector<int>& per_src, int max_in, const MergeLargeLayout& L,
                                 const void* workspace, int64_t workspace_bytes) {
  for (size_t s = 0; s < per_src.size(); ++s)
    if ((long)per_src[s] * max_in > MERGE_LARGE_POOL_CAP)
      return fail(who + ": source " + std::to_string(s) + " has " + std::to_string(per_src[s]) + " views of up to " + std::to_string(max_in) +
                  " rows: above the pool capacity MERGE_LARGE_POOL_CAP = " + std::to_string(MERGE_LARGE_POOL_CAP) + " rows per source");
  if (!workspace) return fail(who + ": the workspace is NULL (" + who + "_bytes gives its size: " + std::to_string(L.bytes) + " bytes)");
  if (workspace_bytes < L.bytes)
    return fail(who + ": the workspace holds " + std::to_string(workspace_bytes) + " bytes, " + who + "_bytes asks for " + std::to_string(L.bytes));
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(who + ": the workspace is not 16-byte aligned");
  return 0;
}

// The view tables of a merge call, uploaded on the context's stream: src_off [n_src + 1] | src_views [n_views] (the views of every source,
// ascending; only when off_dev is asked for: the one-block merge) | MergeView [n_views].  The only wait is for the previous call's upload
// to have left the host copy.
static int merge_upload_tables(sylph_ctx* c, int n_src, int n_views, const int* view_src, const float* view_x0, const float* view_y0,
                               const float* view_w, const int* view_flip, const std::vector<int>& per_src, const int** off_dev,
                               const MergeView** mv_dev, const StitchView* sv_host = nullptr, const StitchView** sv_dev = nullptr) {
  const size_t ints = off_dev ? (size_t)n_src + 1 + n_views : 0, sv_at = ints * sizeof(int) + (size_t)n_views * sizeof(MergeView);
  const size_t need = sv_at + (sv_host ? (size_t)n_views * sizeof(StitchView) : 0);  // (the stitching merge: StitchView [n_views] behind)
  if (c->merge_ev) HIPCHK(hipEventSynchronize(c->merge_ev));
  else HIPCHK(hipEventCreateWithFlags(&c->merge_ev, hipEventDisableTiming));
  if (need > c->merge_tab_cap) {
    if (c->merge_tab) c->dfree(c->merge_tab);
    c->merge_tab = nullptr; c->merge_tab_cap = 0;
    RET(ctx_alloc(c, &c->merge_tab, need * 2));
    c->merge_tab_cap = need * 2;
  }
  c->merge_host.resize(need);
  MergeView* mv = reinterpret_cast<MergeView*>(c->merge_host.data() + ints * sizeof(int));
  for (int v = 0; v < n_views; ++v) mv[v] = MergeView{view_src[v], view_x0[v], view_y0[v], view_w[v], view_flip[v] ? 1 : 0};
  if (off_dev) {
    int* off = reinterpret_cast<int*>(c->merge_host.data());
    int* list = off + n_src + 1;
    off[0] = 0;
    for (int s = 0; s < n_src; ++s) off[s + 1] = off[s] + per_src[s];
    std::vector<int> fill(off, off + n_src);
    for (int v = 0; v < n_views; ++v) list[fill[view_src[v]]++] = v;
  }
  if (sv_host) {
    memcpy(c->merge_host.data() + sv_at, sv_host, (size_t)n_views * sizeof(StitchView));
    *sv_dev = reinterpret_cast<const StitchView*>(reinterpret_cast<const char*>(c->merge_tab) + sv_at);
  }
  HIPCHK(hipMemcpyAsync(c->merge_tab, c->merge_host.data(), need, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->merge_ev, c->stream));
  if (off_dev) *off_dev = reinterpret_cast<const int*>(c->merge_tab);
  *mv_dev = reinterpret_cast<const MergeView*>(reinterpret_cast<const char*>(c->merge_tab) + ints * sizeof(int));
  return 0;
}

/* see include/sylph_hip.h */
int sylph_merge_views(sylph_ctx* c, int n_src, int n_views, const int* view_src, const float* view_x0, const float* view_y0, const float* view_w,
                      const int* view_flip, int max_in, const float* boxes, const float* scores, const int* classes, const int* counts, int max_out,
                      float* out_boxes, float* out_scores, int* out_classes, int* out_view, int* out_row, int* out_counts, int* status) {
  std::vector<int> per_src;
  RET(merge_check_views("sylph_merge_views", n_src, n_views, view_src, view_x0, view_y0, view_w, view_flip, max_in, max_out,
                        boxes && scores && classes && counts && out_boxes && out_scores && out_classes && out_view && out_row && out_counts && status,
                        &per_src));
  int max_views = 0;
  for (int s = 0; s < n_src; ++s) {
    if ((long)per_src[s] * max_in > MERGE_POOL_CAP)
      return fail("sylph_merge_views: source " + std::to_string(s) + " has " + std::to_string(per_src[s]) + " views of up to " + std::to_string(max_in) +
                  " rows: above the pool capacity MERGE_POOL_CAP = " + std::to_string(MERGE_POOL_CAP) + " rows per source");
    max_views = per_src[s] > max_views ? per_src[s] : max_views;
  }
  HIPCHK(hipSetDevice(c->device));
  const int* off_dev;
  const MergeView* mv_dev;
  RET(merge_upload_tables(c, n_src, n_views, view_src, view_x0, view_y0, view_w, view_flip, per_src, &off_dev, &mv_dev));
  const float thr = c->cfg.nms_thresh;
  const int K = c->cfg.post_nms_topk, pool_max = max_views * max_in;
  KCHK(timed_op(c, "merge_views_kernel", 0.0, c->stream, [=](hipStream_t st) {
         return launch_merge_views(n_src, off_dev, off_dev + n_src + 1, mv_dev, max_views, pool_max, max_in, boxes, scores, classes, counts, thr, K,
                                   max_out, out_boxes, out_scores, out_classes, out_view, out_row, out_counts, status, st);
       }), "merge_views");
  return 0;
}

/* see include/sylph_hip.h */
int64_t sylph_merge_views_large_bytes(int n_src, int n_views, int max_in) {
  return merge_workspace_bytes("sylph_merge_views_large_bytes", merge_large_layout(n_src, n_views, max_in), n_src, n_views, max_in);
}

/* see include/sylph_hip.h */
int sylph_merge_views_large(sylph_ctx* c, int n_src, int n_views, const int* view_src, const float* view_x0, const float* view_y0,
                            const float* view_w, const int* view_flip, int max_in, const float* boxes, const float* scores, const int* classes,
                            const int* counts, int topk, int max_out, float* out_boxes, float* out_scores, int* out_classes, int* out_view,
                            int* out_row, int* out_counts, int* status, void* workspace, int64_t workspace_bytes) {
  const std::string who = "sylph_merge_views_large";
  std::vector<int> per_src;
  RET(merge_check_views(who, n_src, n_views, view_src, view_x0, view_y0, view_w, view_flip, max_in, max_out,
                        boxes && scores && classes && counts && out_boxes && out_scores && out_classes && out_view && out_row && out_counts && status,
                        &per_src));
  RET(merge_check_topk(who, topk));
  RET(merge_check_workspace(who, per_src, max_in, merge_large_layout(n_src, n_views, max_in), workspace, workspace_bytes));
  HIPCHK(hipSetDevice(c->device));
  const MergeView* mv_dev;
  RET(merge_upload_tables(c, n_src, n_views, view_src, view_x0, view_y0, view_w, view_flip, per_src, nullptr, &mv_dev));
  const float thr = c->cfg.nms_thresh;
  const int K = topk < 0 ? c->cfg.post_nms_topk : topk;
  KCHK(timed_op(c, "merge_large_kernels", 0.0, c->stream, [=](hipStream_t st) {
         return launch_merge_views_large(n_src, n_views, mv_dev, max_in, boxes, scores, classes, counts, thr, K, max_out, out_boxes, out_scores,
                                         out_classes, out_view, out_row, out_counts, status, workspace, st);
       }), "merge_views_large");
  return 0;
}

/* see include/sylph_hip.h */
int64_t sylph_stitch_views_bytes(int n_src, int n_views, int max_in) {
  return merge_workspace_bytes("sylph_stitch_views_bytes", stitch_layout(n_src, n_views, max_in), n_src, n_views, max_in);
}

/* see include/sylph_hip.h */
int sylph_stitch_views(sylph_ctx* c, int n_src, int n_views, const int* view_src, const float* view_x0, const float* view_y0,
                       const float* view_w, const float* view_h, const int* view_flip, const float* src_w, const float* src_h, int max_in,
                       const float* boxes, const float* scores, const int* classes, const int* counts, float stitch_thr, float border_px,
                       int topk, int max_out, float* out_boxes, float* out_scores, int* out_classes, int* out_view, int* out_row,
                       int* out_stitched, int* out_counts, int* status, void* workspace, int64_t workspace_bytes) {
  const std::string who = "sylph_stitch_views";
  std::vector<int> per_src;
  RET(merge_check_views(who, n_src, n_views, view_src, view_x0, view_y0, view_w, view_flip, max_in, max_out,
                        boxes && scores && classes && counts && out_boxes && out_scores && out_classes && out_view && out_row && out_stitched &&
                            out_counts && status,
                        &per_src));
  if (!view_h || !src_w || !src_h) return fail(who + ": a view table is NULL");
  if (!(stitch_thr > 0.f && stitch_thr <= 1.f)) return fail(who + ": stitch_thr " + std::to_string(stitch_thr) + " is outside (0, 1]");
  if (!(border_px >= 0.f)) return fail(who + ": border_px " + std::to_string(border_px) + " must be at least 0");
  RET(merge_check_topk(who, topk));
  for (int s = 0; s < n_src; ++s)
    if (!(src_w[s] > 0.f && src_h[s] > 0.f))
      return fail(who + ": source " + std::to_string(s) + " is " + std::to_string(src_w[s]) + " x " + std::to_string(src_h[s]) + ": sizes must be positive");
  std::vector<StitchView> sv((size_t)n_views);
  for (int v = 0; v < n_views; ++v) {
    const int s = view_src[v];
    if (!(view_w[v] > 0.f && view_h[v] > 0.f))
      return fail(who + ": the crop of view " + std::to_string(v) + " is " + std::to_string(view_w[v]) + " x " + std::to_string(view_h[v]) +
                  ": sizes must be positive");
    if (!(view_x0[v] >= 0.f && view_y0[v] >= 0.f && view_x0[v] + view_w[v] <= src_w[s] && view_y0[v] + view_h[v] <= src_h[s]))
      return fail(who + ": the crop of view " + std::to_string(v) + ", (" + std::to_string(view_x0[v]) + ", " + std::to_string(view_y0[v]) + ") + " +
                  std::to_string(view_w[v]) + " x " + std::to_string(view_h[v]) + ", leaves its " + std::to_string(src_w[s]) + " x " +
                  std::to_string(src_h[s]) + " source");
    sv[v] = StitchView{view_h[v], src_w[s], src_h[s]};
  }
  RET(merge_check_workspace(who, per_src, max_in, stitch_layout(n_src, n_views, max_in), workspace, workspace_bytes));
  HIPCHK(hipSetDevice(c->device));
  const MergeView* mv_dev;
  const StitchView* sv_dev;
  RET(merge_upload_tables(c, n_src, n_views, view_src, view_x0, view_y0, view_w, view_flip, per_src, nullptr, &mv_dev, sv.data(), &sv_dev));
  const float thr = c->cfg.nms_thresh;
  const int K = topk < 0 ? c->cfg.post_nms_topk : topk;
  KCHK(timed_op(c, "stitch_kernels", 0.0, c->stream, [=](hipStream_t st) {
         return launch_stitch_views(n_src, n_views, mv_dev, sv_dev, max_in, boxes, scores, classes, counts, thr, stitch_thr, border_px, K, max_out,
                                    out_boxes, out_scores, out_classes, out_view, out_row, out_stitched, out_counts, status, workspace, st);
       }), "stitch_views");
  return 0;
}

}  // extern "C"
