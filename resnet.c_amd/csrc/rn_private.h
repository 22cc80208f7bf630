/* rn_private.h -- library-internal functions that cross the C / HIP boundary (plain C).
 *
 * None of them is part of the C-ABI of rn_hip.h and none is exported.  Both the file that
 * defines a function and the files that call it include this header, so a signature that
 * drifts fails to compile instead of linking and misbehaving. */
#ifndef RN_PRIVATE_H
#define RN_PRIVATE_H

#include "rn_hip.h"
#include "rn_operands.h"
#include "rn_params.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- rn_ctx.hip: rn_model.c is plain C and sees the context only through functions ---- */
int rn_ctx_graphs_live(const rn_ctx *ctx);
/* rn_ctx_set_tap_skip's mode of a context (the model gives it to the contexts of its other streams) */
int rn_ctx_tap_skip_mode(const rn_ctx *ctx);
/* everything queued on ctx's stream after this call waits for the event (the stream, not the host) */
int rn_ctx_wait_event(rn_ctx *ctx, rn_event *ev);
int rn_ctx_scratch_slot(rn_ctx *ctx, int slot, uint64_t bytes, void **ptr);
int rn_ctx_is_capturing(rn_ctx *ctx);
/* sets the text rn_last_error returns; returns status */
int rn_ctx_set_error(rn_ctx *ctx, int status, const char *msg);
/* pageable host memory -> device on the context's stream, over when the call returns */
int rn_ctx_upload_sync(rn_ctx *ctx, void *dev, const void *host, uint64_t bytes);

/* ---- rn_conv.hip / rn_head.hip: kernels only the model driver launches ---- */
/* rn_linear_forward through the direct kernel whatever the alignment (class counts that are no multiple of 4) */
int rn_linear_direct_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight, const float *bias,
                             uint64_t B, uint64_t in_features, uint64_t out_features);
/* n bf16 values as fp32 (exact): the pooled features of a bf16 model */
int rn_widen_bf16_forward(rn_ctx *ctx, const void *src_bf16, float *dst, uint64_t n);

/* ---- dilated convolution: the public entry points (rn_conv.hip) have checked the dilation and the output size ---- */
/* rn_conv2d_nhwc_forward_dt with a dilation (rn_conv.hip): the dense contraction, also of a bf16 grouped panel */
int rn_conv_dense_nhwc_forward_dt(rn_ctx *ctx, int dtype, int out_dtype, const void *inp, void *out,
                                  const void *packed_weight, uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                  uint64_t dilation, uint64_t h_out, uint64_t w_out, uint64_t B, uint64_t in_channels,
                                  uint64_t out_channels, uint64_t H, uint64_t W, const rn_epilogue *epilogue);
/* rn_conv2d_grouped_forward / rn_conv2d_grouped_nhwc_forward_dt with a dilation (rn_conv_group.hip) */
int rn_conv_group_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight, uint64_t kernel_size,
                          uint64_t stride, uint64_t padding, uint64_t dilation, uint64_t h_out, uint64_t w_out,
                          uint64_t B, uint64_t in_channels, uint64_t out_channels, uint64_t H, uint64_t W,
                          uint64_t groups);
int rn_conv_group_nhwc_forward_dt(rn_ctx *ctx, int dtype, int out_dtype, const void *inp, void *out,
                                  const void *packed_weight, uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                  uint64_t dilation, uint64_t h_out, uint64_t w_out, uint64_t B, uint64_t in_channels,
                                  uint64_t out_channels, uint64_t H, uint64_t W, uint64_t groups,
                                  const rn_epilogue *epilogue);

/* ---- rn_stage.hip: what every object behind the backbone (neck, rpn, box head, mask head, segmentation head) is made
 * of.  An object declares its parameters (rn_params.h) at create time, its convolution units and its scratch tensors;
 * set_tensor, the "is not set" walk, the pack, the growth guard and the frees are here, once. ---- */
/* the whole of a *_set_tensor behind its NULL-object check, under the name fn; `what`: "the neck", "the rpn", ...
 * Keeps a host copy; nothing touches the device before finalize. */
int rn_stage_set_tensor(rn_ctx *ctx, const char *fn, const char *what, int finalized, rn_params *t, const char *key,
                        const float *host_data, uint64_t numel);
/* RN_OK, or the refusal "<fn>: <key> is not set" for the first entry that is not */
int rn_stage_all_set(rn_ctx *ctx, const char *fn, const rn_params *t);
/* a convolution on the device: its packed panel, the epilogue's scale (a folded batch-norm; else NULL) and shift (that
 * batch-norm's, or the bias), and a second panel where the object has one (a dilated branch's centre tap) */
typedef struct rn_stage_unit {
    void *packed;
    float *scale, *shift;
    void *center;
} rn_stage_unit;
/* Fills u->packed (and shift, scale) from host tensors: w [cout, cin, k, k] as it is stored, and either bias [cout], or
 * bn: a batch-norm's weight, bias, running_mean, running_var [cout] each, or neither (no shift).  Over when it returns;
 * what u held before is freed, and on failure u holds nothing. */
int rn_stage_pack(rn_ctx *ctx, int dtype, const float *w, uint64_t cin, uint64_t cout, uint64_t k, const float *bias,
                  const float *const *bn, rn_stage_unit *u);
void rn_stage_unit_free(rn_ctx *ctx, rn_stage_unit *u);
/* Two linear layers of `len` inputs as ONE panel of P rows: wa [ra, len] above wb [rb, len], zero rows up to P, and
 * behind the panel the P biases likewise (ba, bb, zeros).  The added rows are exact zeros in every sum.  malloc'd
 * (P * len + P values), or NULL. */
float *rn_stage_side_by_side(const float *wa, const float *ba, uint64_t ra, const float *wb, const float *bb, uint64_t rb,
                             uint64_t len, uint64_t P);
/* a scratch tensor of an object: where its pointer lives and the bytes the capacities asked for need (0: none) */
typedef struct rn_scratch_item {
    void **ptr;
    uint64_t bytes;
} rn_scratch_item;
/* The one growth rule, like the model's logits buffer: never on a stream that is being captured (RN_ERR_UNSUPPORTED),
 * never while a captured graph of the context may hold what the object had (any of caps > 0: RN_ERR_INVALID).  Then
 * sync, free the list, allocate the list, caps = want.  A failed allocation leaves caps at 0. */
int rn_stage_grow(rn_ctx *ctx, const char *who, const rn_scratch_item *list, int n, uint64_t *caps, const uint64_t *want,
                  int n_caps);
void rn_stage_free_list(rn_ctx *ctx, const rn_scratch_item *list, int n);

/* ---- rn_seg.hip: the segmentation head as the model driver queues it ---- */
/* 1 when the head is finalized and reads maps of in_channels channels of `dtype`; *why: what is wrong otherwise */
int rn_seg_head_matches(const rn_seg_head *hd, uint64_t in_channels, int dtype, const char **why);
/* in_channels, mid_channels (a DeepLab head: its ASPP width), classes, and classes rounded up to a multiple of 4 (the
 * coarse scores' pixel pitch) */
void rn_seg_head_dims(const rn_seg_head *hd, uint64_t dims[4]);
/* The one source of what a forward of the head launches: returns the number of launches of a forward of B images on
 * an h x w map to H x W (FCN: 3; DeepLab: rates + 8) and, for step 0 .. that - 1, the launch's profile name, FLOPs
 * and bytes (name, flops, bytes: any may be NULL; another step only counts).  A DeepLab branch reports the route
 * that runs at this h x w: a ninth of the FLOPs where the centre-tap plan applies. */
int rn_seg_head_plan(const rn_seg_head *hd, uint64_t B, uint64_t h, uint64_t w, uint64_t H, uint64_t W, int want_scores,
                     int want_labels, int step, const char **name, double *flops, double *bytes);
/* the head's scratch for `images` images of `pixels` coarse pixels (h x w) each; grows under rn_stage_grow's rule */
int rn_seg_head_reserve(rn_seg_head *hd, uint64_t images, uint64_t pixels);
/* launch `step` of rn_seg_head_plan for B images of an h x w map on ctx; their scratch starts img0 images into the
 * head's tensors (img0 * h * w coarse pixels into the per-pixel ones, img0 rows into a DeepLab head's pooled vectors) */
int rn_seg_head_step(rn_seg_head *hd, rn_ctx *ctx, int step, const void *x_nhwc, uint64_t img0, uint64_t B, uint64_t h,
                     uint64_t w, uint64_t H, uint64_t W, float *scores_nchw, uint8_t *labels);

/* ---- rn_fpn.hip: the feature pyramid neck as the model driver queues it ---- */
/* the launches of a neck's forward: the lateral 1x1 of a level, the top-down step from a level into the next finer
 * one (in place on that one's lateral), the 3x3 of a level (fp32 output), the max-pool of the coarsest 3x3 output,
 * the NCHW export of a level's output (level == n_levels: the pooled one) */
enum { RN_FPN_INNER = 0, RN_FPN_TOPDOWN = 1, RN_FPN_LAYER = 2, RN_FPN_POOL = 3, RN_FPN_EXPORT = 4 };
/* 1 when the neck is finalized, stores `dtype` and lives on the device of ctx (its weights and scratch are read by
 * launches on the model's streams); *why: what is wrong otherwise */
int rn_fpn_matches(const rn_fpn *fpn, const rn_ctx *ctx, int dtype, const char **why);
/* levels, extra (0 none, 1 pool), out_channels, in_channels of every level; any pointer may be NULL */
void rn_fpn_dims(const rn_fpn *fpn, int *n_levels, int *extra, uint64_t *out_channels, uint64_t in_channels[4]);
/* the neck's scratch for `images` images whose level i is an h[i] x w[i] map; grows under rn_stage_grow's rule */
int rn_fpn_reserve(rn_fpn *fpn, uint64_t images, const uint64_t *h, const uint64_t *w);
/* FLOPs and bytes of one launch of `kind` at `level` for B images (the profile's figures) */
void rn_fpn_cost(const rn_fpn *fpn, int kind, int level, uint64_t B, const uint64_t *h, const uint64_t *w, double *flops,
                 double *bytes);
/* one launch of `kind` at `level` on ctx for B images whose scratch starts img0 images into the neck's tensors.
 * x_nhwc: the level's map (RN_FPN_INNER only); dst_nchw: where the B images' output goes (RN_FPN_EXPORT only) */
int rn_fpn_step(rn_fpn *fpn, rn_ctx *ctx, int kind, int level, const void *x_nhwc, uint64_t img0, uint64_t B,
                const uint64_t *h, const uint64_t *w, float *dst_nchw);

/* ---- rn_roi.hip / rn_fpn.hip: the pooler behind a neck ---- */
/* rn_roi_align_forward_dt's launch, no checks, for a window of the batch: the maps start at image img_lo and hold
 * img_cnt images; image indices 0 .. images - 1 are valid.  The launch writes the rows of the RoIs whose image is in
 * its window and, with write_invalid, the rows of zeros of the RoIs whose index is invalid; every other row it leaves
 * to the launch of another window. */
int rn_roi_align_window(rn_ctx *ctx, int dtype, uint64_t n_levels, const void *const *x_nhwc, const uint64_t *h,
                        const uint64_t *w, const float *scales, const float *thr, uint64_t images, uint64_t img_lo,
                        uint64_t img_cnt, int write_invalid, uint64_t C, const float *rois_dev, uint64_t K, uint64_t PH,
                        uint64_t PW, int sampling_ratio, int aligned, float *out, int32_t *levels_out);
/* the same window of rn_roi_align_nhwc_forward_dt: out [K, PH, PW, C] on a 16-byte boundary */
int rn_roi_align_nhwc_window(rn_ctx *ctx, int dtype, uint64_t n_levels, const void *const *x_nhwc, const uint64_t *h,
                             const uint64_t *w, const float *scales, const float *thr, uint64_t images, uint64_t img_lo,
                             uint64_t img_cnt, int write_invalid, uint64_t C, const float *rois_dev, uint64_t K, uint64_t PH,
                             uint64_t PW, int sampling_ratio, int aligned, float *out, int32_t *levels_out);

/* ---- rn_mask.hip: the windows the parts of a forward use, no checks ---- */
/* rn_detection_rois_forward for the B images from image img0 on; boxes, labels and rois point at these images' rows */
int rn_detection_rois_window(rn_ctx *ctx, const float *boxes, const int32_t *labels, uint64_t img0, uint64_t B, uint64_t D,
                             float *rois);

/* ---- rn_rpn.hip: the RPN behind a neck (its parameters, units and scratch: rn_stage.hip) ---- */
/* 1 when the rpn is finalized, lives on ctx's device, reads in_channels channels and n_levels levels; *why otherwise */
int rn_rpn_matches(const rn_rpn *rpn, const rn_ctx *ctx, uint64_t in_channels, uint64_t n_levels, const char **why);
/* the object's scratch for `images` images whose level l is h[l] x w[l], and pre candidates per (image, level) */
int rn_rpn_reserve(rn_rpn *rpn, uint64_t images, const uint64_t *h, const uint64_t *w, uint64_t pre);
/* every refusal that concerns the request alone, for a forward of `images` images (text in ctx) */
int rn_rpn_check(const rn_rpn *rpn, rn_ctx *ctx, const rn_rpn_request *req, uint64_t images, const uint64_t *h,
                 const uint64_t *w, uint64_t image_h, uint64_t image_w);
/* the request's 11 buffers for `images` images as operands, all of them outputs; returns 11 */
enum { RN_RPN_OPERANDS = 11 };
int rn_rpn_operands(const rn_rpn *rpn, const rn_rpn_request *req, uint64_t images, rn_operand ops[RN_RPN_OPERANDS]);
/* the stage's 2 L + 3 launches on ctx for the B images from the caller's image img0 on, whose scratch starts sub0
 * images into the object's tensors; x: the L fp32 NHWC levels of these B images */
int rn_rpn_step(rn_rpn *rpn, rn_ctx *ctx, const float *const *x, uint64_t sub0, uint64_t img0, uint64_t B,
                const uint64_t *h, const uint64_t *w, uint64_t image_h, uint64_t image_w, const rn_rpn_request *req);

/* ---- rn_detect.hip: the box head behind the pooler (its parameters, units and scratch: rn_stage.hip) ---- */
/* 1 when the box head is finalized, lives on ctx's device and reads in_features values per RoI; *why otherwise */
int rn_box_head_matches(const rn_box_head *bh, const rn_ctx *ctx, uint64_t in_features, const char **why);
/* the object's scratch for `images` images of R RoIs each */
int rn_box_head_reserve(rn_box_head *bh, uint64_t images, uint64_t R);
/* every refusal that concerns the request alone, for a forward of `images` images of R RoIs (text in ctx) */
int rn_box_head_check(const rn_box_head *bh, rn_ctx *ctx, const rn_detect_request *req, uint64_t images, uint64_t R,
                      uint64_t image_h, uint64_t image_w);
/* the request's 9 outputs for `images` images of R RoIs as operands; returns 9 */
enum { RN_BOX_HEAD_OPERANDS = 9 };
int rn_box_head_operands(const rn_box_head *bh, const rn_detect_request *req, uint64_t images, uint64_t R,
                         rn_operand ops[RN_BOX_HEAD_OPERANDS]);
/* the stage's launches (three contractions of one or two launches each, then three) on ctx for the B images from the caller's image img0 on, whose scratch starts sub0 images
 * into the object's tensors; pooled [B*R, in_features] and rois [B*R, 5]: the rows of these B images */
int rn_box_head_step(rn_box_head *bh, rn_ctx *ctx, const float *pooled, const float *rois, uint64_t sub0, uint64_t img0,
                     uint64_t B, uint64_t R, uint64_t image_h, uint64_t image_w, const rn_detect_request *req);

/* ---- rn_stage.hip: the RoI tower under the mask head and the keypoint head.  Pooled [K, M, M, Cin] through n_layers
 * 3x3 convolutions with bias and ReLU over two ping-pong maps, then ONE 1x1 panel that stands for the head's transposed
 * convolution; behind a neck the RoI former and the NHWC pooler in front.  A head embeds one tower, sets what differs
 * (name .. extra_floats) at create time and keeps only its predictor. ---- */
enum { RN_TOWER_MAX_LAYERS = 8, RN_TOWER_ROWS = 0, RN_TOWER_POOL = 1, RN_TOWER_SCRATCH = 6 };
typedef struct rn_roi_tower {
    rn_ctx *ctx;
    const char *name, *what;            /* the words of its messages: "rn_mask_head", "the mask head" */
    uint64_t Cin, n_layers, ch[RN_TOWER_MAX_LAYERS], M, widest;
    uint64_t panel;                     /* the panel's output channels */
    int panel_relu;                     /* the panel's epilogue has ReLU (its shift: whatever the head packed) */
    uint64_t extra_floats;              /* one further scratch tensor of so many floats per pooled pixel, or 0 */
    int finalized;
    rn_params params;                   /* layer i: 2i, 2i + 1; the head's predictor entries behind them, from 2n on */
    rn_stage_unit unit[RN_TOWER_MAX_LAYERS + 1]; /* the 3x3 layers, then the panel Clast -> panel */
    /* scratch for cap rows: two ping-pong maps [., M, M, widest], the panel's output [., M, M, panel], the extra tensor */
    float *ping, *pong, *t, *extra;
    float *rois, *pooled;               /* behind a neck: the RoI rows [., 5] and the pooled features [., M, M, Cin] of cap_pool rows */
    uint64_t cap[2];                    /* rows (RN_TOWER_ROWS), of them with RoI rows and pooled features (RN_TOWER_POOL) */
} rn_roi_tower;
/* the spelling of layer i's tensor `leaf` ("weight", "bias"); alt: another spelling, or "" */
typedef void (*rn_roi_tower_key)(int layer, const char *leaf, char key[RN_PARAM_KEY], char alt[RN_PARAM_KEY]);
/* The refusals of a head's create under the name fn, in their order: in_channels, n_layers, layer_channels, then `own`
 * (the head's own refusal, or NULL: it always stood here), then resolution against the head's limit. */
int rn_roi_tower_check(rn_ctx *ctx, const char *fn, uint64_t in_channels, uint64_t n_layers, const uint64_t *layer_channels,
                       const char *own, uint64_t resolution, uint64_t max_resolution);
/* a zeroed tower whose name .. extra_floats the head has set: the shapes, ch and widest, the prefix "roi_heads." and the
 * 2 n_layers layer entries of the parameter table (the head adds its predictor's behind them) */
void rn_roi_tower_init(rn_roi_tower *t, rn_ctx *ctx, uint64_t in_channels, uint64_t n_layers, const uint64_t *layer_channels,
                       uint64_t resolution, rn_roi_tower_key key);
/* the front of a finalize under the name fn: "is not set", then the n_layers packs */
int rn_roi_tower_pack_layers(rn_roi_tower *t, const char *fn);
/* the head's reordered transposed convolution as the panel: w [panel, Clast], shift [panel] or NULL */
int rn_roi_tower_pack_panel(rn_roi_tower *t, const float *w, const float *shift);
/* the scratch, the host copies and the units; the context is idle */
void rn_roi_tower_free(rn_roi_tower *t);
/* 1 when the tower is finalized, lives on ctx's device and reads in_channels channels per pooled pixel; *why: what is
 * wrong otherwise, to stand behind "the mask" / "the keypoint" ("head is not finalized") */
int rn_roi_tower_matches(const rn_roi_tower *t, const rn_ctx *ctx, uint64_t in_channels, const char **why);
/* the scratch for `rows` detections (rn_stage_grow's rule); with_pool: the RoI rows and the pooled features of a stage
 * behind a neck as well */
int rn_roi_tower_reserve(rn_roi_tower *t, uint64_t rows, int with_pool);

/* the pooler's fields of a head's request (the public request structs hold them in different places) */
typedef struct rn_roi_pool_view {
    int n_levels;
    const int *level;
    int sampling_ratio, aligned;
    double canonical_scale;
    int canonical_level;
    float *rois, *pooled;               /* the request's outputs [rows, 5] and [rows, M, M, Cin], or NULL */
} rn_roi_pool_view;
/* A RoI head as the neck call and the tower's two forwards see it: the tower, the pooler's view, and the three things
 * that differ between heads.  rn_mask_head_slot / rn_keypoint_head_slot fill it (tower NULL: no such head). */
enum { RN_ROI_HEAD_OPERANDS = 5 };
typedef struct rn_roi_head {
    const char *who, *stage;            /* "mask", "keypoint" in the refusals; the stage's profile name ("mask_stage") */
    rn_roi_tower *tower;
    const void *head, *req;             /* the head's own: what the three functions read */
    rn_roi_pool_view pool;
    /* every refusal that concerns the request's outputs and the shapes alone, for `rows` detections (text in ctx, under
     * fn); boxes_given: the caller has the boxes a paste or a search needs */
    int (*check)(const struct rn_roi_head *s, rn_ctx *ctx, const char *fn, uint64_t rows, int boxes_given, uint64_t image_h,
                 uint64_t image_w);
    /* the request's 5 outputs for `rows` detections as operands, rois and pooled first; returns 5 */
    int (*operands)(const struct rn_roi_head *s, uint64_t rows, uint64_t image_h, uint64_t image_w, rn_operand ops[RN_ROI_HEAD_OPERANDS]);
    /* the launches behind the tower for K detections from row row0 of the request's outputs on: t and extra are the
     * panel's output and the extra tensor of these rows; labels and boxes point at these rows */
    int (*behind)(const struct rn_roi_head *s, rn_ctx *ctx, const float *t, float *extra, const int32_t *labels, const float *boxes,
                  uint64_t row0, uint64_t K, uint64_t image_h, uint64_t image_w);
    float scales[4], thr[3];            /* rn_neck_check: the pooler's levels' scales and the thresholds between them */
} rn_roi_head;
void rn_mask_head_slot(rn_mask_head *mh, const rn_mask_request *req, rn_roi_head *s);
void rn_keypoint_head_slot(rn_keypoint_head *kh, const rn_keypoint_request *req, rn_roi_head *s);
/* The head's launches on ctx for K detections whose scratch starts sub0 rows into the tower's tensors: n_layers + 1
 * contractions of one or two launches, then the head's own.  ctx->layout is NHWC. */
int rn_roi_head_step(const rn_roi_head *s, rn_ctx *ctx, const float *pooled_nhwc, const int32_t *labels, const float *boxes,
                     uint64_t sub0, uint64_t row0, uint64_t K, uint64_t image_h, uint64_t image_w);
/* The stage behind a neck for the B images from the caller's image img0 on (D detections each), whose scratch starts
 * sub0 images into the tower's tensors: the RoI former on these images' detection rows, the NHWC pooler on maps[i]
 * (level i of image img0, h[i] x w[i], fp32), then rn_roi_head_step.  boxes [images*D, 4], labels [images*D] and the
 * request's outputs: the whole call's. */
int rn_roi_head_stage(const rn_roi_head *s, rn_ctx *ctx, const void *const *maps, const uint64_t *h, const uint64_t *w,
                      uint64_t images, uint64_t sub0, uint64_t img0, uint64_t B, uint64_t D, const float *boxes,
                      const int32_t *labels, uint64_t image_h, uint64_t image_w);
/* The frame of a stand-alone *_forward under the name fn, behind the head's own request check: pooled_nhwc's NULL
 * refusal, `own` (the head's refusal that stands here, or NULL), its alignment, the operand list, the reserve, and the
 * step with ctx->layout NHWC around it. */
int rn_roi_head_forward(const rn_roi_head *s, const char *fn, const float *pooled_nhwc, const char *own, const rn_operand *ops,
                        int n_ops, const int32_t *labels, const float *boxes, uint64_t K, uint64_t image_h, uint64_t image_w);

/* ---- rn_fpn.hip: one forward of a neck and what runs behind it, for both entry families ---- */
/* The description of a call.  It lives on the stack of the entry point that runs it (rn_fpn_forward*, the model's
 * forward_fpn); rn_neck_check fills the second half (and the heads' scales and thresholds) once and everything after
 * it only reads. */
enum { RN_NECK_MASK_SLOT = 0, RN_NECK_KEYPOINT_SLOT = 1, RN_NECK_HEADS = 2 };
typedef struct rn_neck_call {
    /* what the caller gave */
    rn_fpn *fpn;
    float *const *out;              /* n + extra NCHW outputs; NULL: that level is not exported */
    const rn_roi_pool *roi;         /* the pooler behind the neck, or NULL */
    rn_rpn *rpn;                    /* the rpn behind the neck and its request, or NULL */
    const rn_rpn_request *rpn_req;
    rn_box_head *box_head;          /* the box head behind the chained pooler and its request, or NULL */
    const rn_detect_request *det_req;
    rn_roi_head head[RN_NECK_HEADS]; /* the RoI heads behind the box head and their requests (tower NULL: none) */
    uint64_t image_h, image_w;      /* the image the rpn and the box head clip to */
    uint64_t h[4], w[4];            /* the input levels' maps */
    uint64_t images;                /* the batch of the whole call */
    /* what rn_neck_check derives */
    int n, extra;
    uint64_t a, hl[5], wl[5];       /* out_channels; the output levels' maps (the pooled one last) */
    int chain;                      /* the pooler pools the proposals this call writes, every part its own rows */
    int pool;                       /* the max-pool runs */
    int layer_runs[4];              /* the 3x3 of the level runs: exported, pooled from, or read by the pooler / the rpn */
    float scales[4], thr[3];        /* the pooler's levels' scales and the thresholds between them */
} rn_neck_call;
/* Every refusal the two families share, in one order: the neck, the outputs' alignment, nothing wanted, the pooler's
 * request, the rpn and its request, the box head's conditions and request, the mask head's, the keypoint head's, then the operand matrix: no
 * output of the exported levels, the pooler, the rpn, the box head, the mask head, the keypoint head or `others` (the family's own operands: the model's head outputs,
 * the stand-alone family's input maps) may share a byte with an operand of another of these groups -- but for the
 * chained pooler's rois_dev, which IS the rpn's out.rois.  Text in ctx, under the name fn; nothing is launched. */
int rn_neck_check(rn_neck_call *call, rn_ctx *ctx, const char *fn, const rn_operand *others, int n_others);
/* the scratch of the neck, the rpn, the box head, the mask head and the keypoint head for parts of at most images_at_once images */
int rn_neck_reserve(const rn_neck_call *call, uint64_t images_at_once);
/* The one source of what follows the laterals for a part of B images: returns the number of steps and, for step
 * 0 .. that - 1, its profile name, layer, FLOPs and bytes (any may be NULL; another step only counts).  In order:
 * the top-down steps coarsest first, the 3x3 of every level that runs, the pool, the exports, the rpn's stage, the
 * pooler (the whole call's window, or in the chain the part's own rows), the box head's stage, the mask head's stage, the keypoint head's stage. */
int rn_neck_plan(const rn_neck_call *call, uint64_t B, int step, const char **op, const char **layer, double *flops,
                 double *bytes);
/* launch `step` of rn_neck_plan on ctx for the B images from the caller's image img0 on, whose scratch starts sub0
 * images into the objects' tensors */
int rn_neck_step(const rn_neck_call *call, rn_ctx *ctx, int step, uint64_t sub0, uint64_t img0, uint64_t B);
/* the profile name of a neck's launch (a record keeps the pointer: literals) */
const char *rn_fpn_op_name(const rn_fpn *fpn, int kind, int level);

/* ---- rn_stem.hip ---- */
/* 1 when the fused stem + max-pool launch takes a padded image of Hp x Wp (nchw: the NCHW-fetching form on
 * an image of Hp - 6 x Wp - 6) of `dtype`: its documented conditions on the geometry alone */
int rn_stem_pool_applies(int dtype, uint64_t Hp, uint64_t Wp, int nchw);

/* ---- rn_model.c: what the pipeline and the graph capture (rn_pipeline.hip) need of a model ---- */
/* the model keeps its context private; the pipeline queues on its compute stream */
rn_ctx *rn_model_context(rn_model *m);
int rn_model_profiling_enabled(const rn_model *m);
/* every context the model has queued batch parts on so far; returns how many were written to out */
int rn_model_contexts(rn_model *m, rn_ctx **out, int cap);
/* rn_model_capture / rn_graph_destroy count the graphs that hold the model */
void rn_model_graph_ref(rn_model *m, int delta);
/* rn_pipeline_create* / rn_pipeline_destroy count the pipelines whose buffers are sized for the model's input
 * (rn_model_set_input_size is refused while one lives).  attach returns the counter's cell, which outlives the
 * model when the model is destroyed first; detach takes that cell, not the model. */
void *rn_model_pipeline_attach(rn_model *m);
void rn_model_pipeline_detach(void *cell);
/* decoded images whose resize tables are on the device already */
int rn_model_forward_images_table(rn_model *m, const uint8_t *packed_dev, const void *table_dev, uint64_t B,
                                  double src_bytes, float *logits, int mode);

#ifdef __cplusplus
}
#endif

#endif /* RN_PRIVATE_H */
