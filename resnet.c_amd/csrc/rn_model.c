/*
 * rn_model.c -- the network driver, plain C over the C-ABI of rn_hip.h.
 *
 * Replaces the reference driver cuda/inference/main.cu:
 *   createLayer / createResnet152   main.cu:53-89,109-125  -> rn_model_create + set_tensor/load_dir
 *   layerForward                    main.cu:127-166        -> block_forward
 *   resnet152Forward                main.cu:168-226        -> rn_model_forward (run_front, run_blocks, run_head)
 * generalised over the block counts (ResNet-50/101/152) and the batch size, plus the basic-block
 * networks ResNet-18/34 (torchvision's layout: two 3x3 convolutions per block, expansion 1; the
 * reference ships bottleneck networks only).
 *
 * Differences that are deliberate (MI355X-first):
 *   - activations are NHWC inside; the NCHW input image is converted once (to a
 *     4-channel zero-padded NHWC image the stem contraction reads);
 *   - no device synchronisation between ops: everything is queued on the
 *     context's stream (the reference syncs after every launch, nn.cu:14-85);
 *   - activation buffers are a fixed set of ping-pong arenas sized for the largest
 *     batch seen, instead of one cached tensor per block (main.cu:141-159): the
 *     same "second forward allocates nothing" behaviour with ~3x less memory;
 *   - the unused device-to-host copy of the layer4 activation (main.cu:207) is gone;
 *   - RN_FWD_FUSED folds batch-norm, ReLU and the residual add into the
 *     contraction's epilogue; RN_FWD_REFERENCE_OPS launches one kernel per reference
 *     op in the reference's order (conv, bn in place, relu in place, add into act3,
 *     relu), which is the parity baseline for the fused path.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rn_hip.h"
#include "rn_private.h"

#define RN_MAX_KEY 96
/* RGB images of the model's H x W (rn_model_set_input_size; the default below), a 64-channel stem; the size and
 * the class count are fields of the model */
#define RN_DEFAULT_SIDE 224
#define RN_MIN_SIDE 32
#define RN_MAX_SIDE 2048
#define RN_RESIZE_SIDE 256 /* decoded images: the shorter side before the centre crop (to RN_DEFAULT_SIDE) */
#define RN_STEM_WIDTH 64
#define RN_DEFAULT_CLASSES 1000
#define RN_MAX_CLASSES 65536

#define RN_MAX_STREAMS 4

typedef struct {
    char key[RN_MAX_KEY];
    uint64_t numel;
    float *dev;
    int is_set;
} rn_param;

typedef struct {
    char name[RN_MAX_KEY];
    uint64_t cin, cout, k, stride, pad;
    uint64_t dil;                  /* dilation: 1 but for conv2 of a dilated stage (rn_model_set_dilation) */
    uint64_t groups;               /* > 1: a grouped convolution (ResNeXt's conv2), weight [cout][cin/groups][k][k] */
    int w, bn_w, bn_b, bn_m, bn_v; /* indices into params */
    void *packed;                  /* K-major panel, model dtype */
    float *scale, *shift;          /* folded batch-norm */
    /* tuned contraction tile (0 = per-launch choice) and the launch batch it was tuned at: slot 0
     * for the parts a batch runs as on its streams, slot 1 for the whole (sub-)batch on one stream
     * (profiled forwards, rn_model_set_streams(m, 1)) */
    int tile[2];
    uint64_t tile_B[2];
} rn_conv;

typedef struct {
    char name[RN_MAX_KEY];
    int conv1, conv2, conv3, ds; /* indices into convs; ds = -1 when absent, conv3 = -1 in a basic block */
    int tail;                    /* the convolution that carries the residual: conv3, or conv2 of a basic block */
    /* blocks with a downsample branch: the tail convolution and downsample as one contraction
     * (rn_conv2d_nhwc_pair_forward_dt): rows [Cout][K3 + Kd] with both batch-norm scales
     * folded in, and the sum of the two shifts */
    void *pair_packed;
    float *pair_shift;
    int pair_tile[2];
    uint64_t pair_tile_B[2];
} rn_block;

typedef struct {
    const char *op;
    char layer[RN_MAX_KEY];
    double flops, bytes;
    rn_event *start, *stop;
    float ms;
} rn_prof;

/* One contraction launch: what op_conv / op_pair build and launch_call runs, in a forward and again,
 * from the call list, when the tiles are tuned. */
typedef struct {
    int conv;       /* the convolution; of a pair, its tail */
    int pair_block; /* >= 0: the fused tail + downsample call of that block (x2, H2, W2) */
    int exact;      /* the stem in its exact-K form (x = physically padded image) */
    const void *x, *x2;
    void *y;
    uint64_t B, H, W, pad, H2, W2; /* H, W: the input's; the output size follows from them and pad */
    rn_epilogue ep;
    int has_ep;
} rn_conv_call;

/* What the ops of the forward_sub call being queued run on: set by run_begin, nowhere else. */
typedef struct {
    rn_ctx *ctx;
    int mode;
    int t1_ready; /* the previous block's chained launch has produced this block's conv1 output */
    float *x4, *p0, *p1, *dsb, *t1, *t2, *pooled; /* views into the arenas */
    uint64_t img0; /* the caller's index of this launch's first image: sub-batch + part + front slice (stage maps) */
    uint64_t sub0; /* the same image's index inside its sub-batch: its slice of a segmentation head's scratch */
} rn_run;

/* What a pipeline keeps of its model after the model may be gone: freed by whoever leaves last. */
struct rn_model_share {
    int pipelines, model_alive;
};

struct rn_model {
    rn_ctx *ctx;
    int arch;
    int groups, width_per_group; /* torchvision's ResNet arguments: (1, 64) plain, (32, 4) ResNeXt, (1, 128) Wide ... */
    int basic;        /* ResNet-18/34: basic blocks (two 3x3 convolutions, expansion 1) */
    int depths[4];
    uint64_t feat;    /* width of the final feature map: 2048 (bottleneck) or 512 (basic) */
    uint64_t classes; /* rows of fc.weight: 1000 unless rn_model_set_classes said otherwise */
    int classes_locked; /* a tensor was set, a directory loaded or the model finalized: the count stays */
    float *own_logits;  /* [own_logits_cap, classes]: where rn_model_forward_outputs keeps logits nobody asked for */
    uint64_t own_logits_cap;
    int dilate[3];                 /* torchvision's replace_stride_with_dilation: layer2, layer3, layer4 */
    uint64_t H, W;                 /* the input image: 224 x 224 unless rn_model_set_input_size said otherwise */
    uint64_t stem_h, stem_w;       /* the stem's output (112 x 112 at 224) */
    uint64_t pool_h, pool_w;       /* the max-pool's (56 x 56), which the first stage keeps */
    uint64_t max_sub;              /* images per launch batch at this size: see rn_model_forward */
    struct rn_model_share *share;  /* counts the pipelines whose buffers are sized for H x W */
    /* per-image element counts of the arenas (ensure_acts) */
    uint64_t x4_img, p_img, ds_img, t1_img, t2_img;
    uint64_t s1_img; /* the first stage's output per image (56*56*256, or 56*56*64): slices of a depth-first front */
    rn_param *params;
    uint64_t n_params;
    rn_conv *convs;
    int n_convs;
    rn_block *blocks;
    int n_blocks;
    int fc_w, fc_b;
    int finalized;
    int dtype;        /* storage type of activations and packed weights */
    int pair_fusion;  /* fused mode: conv3 + downsample as one contraction (default on) */
    int stem_exact;   /* fp32: stem in the exact-K form, K = 160 instead of 224 (default on) */
    float *stem_packed_exact;
    int graphs_live;         /* graphs captured from this model that still live (rn_model_capture / rn_graph_destroy) */
    int chain;               /* fused bf16 mode: conv3 of a 64- / 128-channel block + conv1 of the next block as one launch (default on) */
    int stem_pool;           /* fused mode: stem + batch-norm + ReLU + max-pool as one launch (default on) */
    uint8_t *crops;          /* [crops_cap,224,224,3]: what rn_model_forward_images_u8 resizes decoded images into */
    uint64_t crops_cap;
    void *stem_pool_packed;  /* its weight panel, model dtype */
    void *fc_packed;  /* fc.weight in the model dtype (bf16 models only) */
    /* activation arenas, sized for batch_cap images */
    uint64_t batch_cap;
    float *x4, *p0, *p1, *dsb, *t1, *t2, *pooled;
    uint64_t act_bytes;
    /* Two halves of a batch on two streams: the launches of one half fill the tails (last
     * round of tiles, prologues, epilogues) of the other's.  Every image's logits are
     * independent of what else is in its launch, so the split changes no bit.  The second
     * stream belongs to a second context on the same device (own scratch). */
    int streams;            /* parts a sub-batch is split into (each >= RN_STREAM_MIN_PART(m) images) */
    rn_ctx *ctxn[RN_MAX_STREAMS - 1];     /* contexts of parts 1.. (part 0 runs on ctx) */
    rn_event *ev_fork, *ev_join[RN_MAX_STREAMS - 1];
    int streams_set;        /* rn_model_set_streams was called: keep it whatever the dtype */
    int single_stream_only; /* tuning pass: its recorded calls are one half */
    /* depth-first front: the stem, the pool and the first stage (the largest tensors) run in
     * front_parts slices of the (sub-)batch, one after the other, so that what one kernel
     * writes is still in the 256 MB Infinity Cache when the next reads it; the rest of the
     * network then runs on the whole batch.  1 = off. */
    int front_parts;
    rn_run run;
    /* rn_model_forward_maps: the stage maps wanted by the call that is running (NULL in every other forward), and
     * the caller's index of the first image of the sub-batch being queued */
    const rn_model_maps *maps;
    uint64_t maps_done;
    /* rn_model_forward_segment: the head and the buffers of the call that is running (NULL in every other forward) */
    rn_seg_head *seg_head;
    const rn_seg_outputs *seg;
    /* rn_model_forward_fpn and what runs behind its neck (rois, proposals, detections): the call that is running, on
     * forward_fpn's stack (NULL in every other forward); its level j reads stage fpn_stage[j] (1..4) */
    const rn_neck_call *neck;
    int fpn_stage[4];
    /* tile tuning: calls of the last forward, and the batch size the tiles were tuned for */
    rn_conv_call *calls;
    int n_calls, cap_calls, recording;
    uint64_t tuned_B;
    int tuned_mode;
    /* profiling */
    int profiling;
    rn_prof *prof;
    uint64_t n_prof, cap_prof;
};

static const uint64_t kWidths[4][3] = {{64, 64, 256}, {256, 128, 512}, {512, 256, 1024},
                                       {1024, 512, 2048}};
static const uint64_t kStrides[4] = {1, 2, 2, 2};
static const uint64_t kBasicWidths[4] = {64, 128, 256, 512};

static int add_param(rn_model *m, const char *key, uint64_t numel)
{
    rn_param *p = &m->params[m->n_params];
    snprintf(p->key, RN_MAX_KEY, "%s", key);
    p->numel = numel;
    p->dev = NULL;
    p->is_set = 0;
    return (int)m->n_params++;
}

static int add_conv_grouped(rn_model *m, const char *name, const char *bn_name, uint64_t cin, uint64_t cout,
                            uint64_t k, uint64_t stride, uint64_t pad, uint64_t groups)
{
    rn_conv *c = &m->convs[m->n_convs];
    char key[RN_MAX_KEY + 16];
    memset(c, 0, sizeof(*c));
    snprintf(c->name, RN_MAX_KEY, "%s", name);
    c->cin = cin;
    c->cout = cout;
    c->k = k;
    c->stride = stride;
    c->pad = pad;
    c->dil = 1;
    c->groups = groups;
    snprintf(key, sizeof(key), "%s.weight", name);
    c->w = add_param(m, key, cout * (cin / groups) * k * k);
    snprintf(key, sizeof(key), "%s.weight", bn_name);
    c->bn_w = add_param(m, key, cout);
    snprintf(key, sizeof(key), "%s.bias", bn_name);
    c->bn_b = add_param(m, key, cout);
    snprintf(key, sizeof(key), "%s.running_mean", bn_name);
    c->bn_m = add_param(m, key, cout);
    snprintf(key, sizeof(key), "%s.running_var", bn_name);
    c->bn_v = add_param(m, key, cout);
    return m->n_convs++;
}

static int add_conv(rn_model *m, const char *name, const char *bn_name, uint64_t cin, uint64_t cout,
                    uint64_t k, uint64_t stride, uint64_t pad)
{
    return add_conv_grouped(m, name, bn_name, cin, cout, k, stride, pad, 1);
}

/* bottleneck width of a stage (torchvision: int(planes * width_per_group / 64) * groups) */
static uint64_t mid_width(const rn_model *m, int li)
{
    return kWidths[li][1] * (uint64_t)m->width_per_group / 64 * (uint64_t)m->groups;
}

/* a convolution's output side */
static uint64_t conv_side(const rn_conv *cv, uint64_t x, uint64_t pad)
{
    return cv->dil > 1 ? rn_conv_output_size_dilated(x, cv->k, cv->stride, pad, cv->dil)
                       : rn_conv_output_size(x, cv->k, cv->stride, pad);
}

/* torchvision's _make_layer with replace_stride_with_dilation, over the blocks of a bottleneck network: a
 * running dilation starts at 1; a flagged stage doubles it and takes stride 1 instead of 2.  Block 0 of a stage
 * runs its conv2 at the stage's stride with the dilation (and padding) from BEFORE the stage, its downsample
 * at the stage's stride; the other blocks run conv2 with the current one.  Weights, panels and folded
 * constants do not depend on any of it. */
static void apply_dilation(rn_model *m)
{
    uint64_t dilation = 1;
    int li, bi, at = 0;
    if (m->basic) return;
    for (li = 0; li < 4; ++li) {
        const uint64_t previous = dilation;
        uint64_t stride = kStrides[li];
        if (li > 0 && m->dilate[li - 1]) {
            dilation *= 2;
            stride = 1;
        }
        for (bi = 0; bi < m->depths[li]; ++bi, ++at) {
            const rn_block *b = &m->blocks[at];
            rn_conv *c2 = &m->convs[b->conv2];
            c2->stride = bi == 0 ? stride : 1;
            c2->dil = c2->pad = bi == 0 ? previous : dilation;
            if (b->ds >= 0) m->convs[b->ds].stride = stride;
        }
    }
}

/* The spatial sizes and, from them, the arenas per image: x4 the input image, p0 / p1 the block outputs
 * (and the stem output), dsb the downsample branch, t1 / t2 the block-internal tensors (a basic block
 * has one: conv1's output).  Max-pool 3x3 s2 p1 (main.cu:114,192); the first stage has stride 1.
 * A bottleneck network takes each arena as the maximum over its stages: undilated that is the stem and the
 * first stage (and layer2.0's conv1), as it always was; a stage that keeps its resolution
 * (rn_model_set_dilation) carries wider tensors on the same map -- layer4's output of a (0,1,1) model at
 * 224 x 224 is 28 x 28 x 2048, twice the stem's. */
#define RN_SUB_BATCH_LIMIT 512
static void set_geometry(rn_model *m, uint64_t H, uint64_t W)
{
    const rn_conv *stem = &m->convs[0];
    /* bf16 and exact-K stems keep a zero border */
    const uint64_t padded = (H + 2 * stem->pad) * (W + 2 * stem->pad);
    uint64_t s1, s2, stem_img, largest;
    m->H = H;
    m->W = W;
    m->stem_h = rn_conv_output_size(H, stem->k, stem->stride, stem->pad);
    m->stem_w = rn_conv_output_size(W, stem->k, stem->stride, stem->pad);
    m->pool_h = rn_conv_output_size(m->stem_h, 3, 2, 1);
    m->pool_w = rn_conv_output_size(m->stem_w, 3, 2, 1);
    s1 = m->pool_h * m->pool_w;
    stem_img = m->stem_h * m->stem_w * stem->cout;
    m->x4_img = padded * 4;
    m->s1_img = s1 * (m->basic ? kBasicWidths[0] : kWidths[0][2]);
    m->p_img = stem_img > m->s1_img ? stem_img : m->s1_img;
    if (m->basic) {
        /* map of the second stage (the 3x3 / 2 / 1 and the 1x1 / 2 / 0 convolutions agree on it) */
        s2 = rn_conv_output_size(m->pool_h, 1, kStrides[1], 0) * rn_conv_output_size(m->pool_w, 1, kStrides[1], 0);
        m->ds_img = s2 * kBasicWidths[1]; /* layer2.0's */
        m->t1_img = s1 * kBasicWidths[0];
        m->t2_img = 0;
    } else {
        uint64_t h = m->pool_h, w = m->pool_w;
        int li;
        m->ds_img = m->t1_img = 0;
        for (li = 0; li < 4; ++li) {
            const uint64_t stride = li > 0 && m->dilate[li - 1] ? 1 : kStrides[li];
            /* (the strided 3x3 with padding == dilation and the 1x1 / stride / 0 agree on the stage's map) */
            const uint64_t ho = rn_conv_output_size(h, 1, stride, 0), wo = rn_conv_output_size(w, 1, stride, 0);
            const uint64_t in = h * w * mid_width(m, li);        /* block 0's conv1 sees the stage's input map */
            const uint64_t out = ho * wo * kWidths[li][2];       /* block outputs, and block 0's downsample branch */
            if (out > m->p_img) m->p_img = out;
            if (out > m->ds_img) m->ds_img = out;
            if (in > m->t1_img) m->t1_img = in;
            if (ho * wo * mid_width(m, li) > m->t1_img) m->t1_img = ho * wo * mid_width(m, li);
            h = ho;
            w = wo;
        }
        m->t2_img = m->t1_img;
    }
    /* The contraction kernels address a tensor with 32-bit byte offsets and refuse one of 2^29 elements or
     * more: a launch batch is the largest power of two, at most 512, whose largest arena tensor stays below
     * that (512 at 224 x 224; 0 = not even one image of this size fits). */
    largest = m->x4_img > m->p_img ? m->x4_img : m->p_img;
    if (m->t1_img > largest) largest = m->t1_img;
    if (m->ds_img > largest) largest = m->ds_img;
    m->max_sub = RN_SUB_BATCH_LIMIT;
    while (m->max_sub > 0 && largest * m->max_sub >= (1ull << 29)) m->max_sub /= 2;
}

static int model_create(rn_ctx *ctx, rn_model **out, int arch, int groups, int width_per_group)
{
    static const int d50[4] = {3, 4, 6, 3}, d101[4] = {3, 4, 23, 3}, d152[4] = {3, 8, 36, 3};
    static const int d18[4] = {2, 2, 2, 2}, d34[4] = {3, 4, 6, 3};
    const int *d;
    rn_model *m;
    int li, bi, total_blocks = 0, max_convs;
    if (!ctx || !out) return RN_ERR_INVALID;
    *out = NULL;
    if (arch == 50) d = d50;
    else if (arch == 101) d = d101;
    else if (arch == 152) d = d152;
    else if (arch == 18) d = d18;
    else if (arch == 34) d = d34;
    else return RN_ERR_UNSUPPORTED;
    m = (rn_model *)calloc(1, sizeof(rn_model));
    if (m) m->pair_fusion = m->stem_exact = 1;
    if (m) m->streams = 2;
    if (m) m->stem_pool = 1;
    if (m) m->chain = 1;
    if (m) m->front_parts = 1;
    if (!m) return RN_ERR_NOMEM;
    m->ctx = ctx;
    m->arch = arch;
    m->groups = groups;
    m->width_per_group = width_per_group;
    m->basic = arch == 18 || arch == 34;
    m->feat = m->basic ? kBasicWidths[3] : kWidths[3][2];
    for (li = 0; li < 4; ++li) {
        m->depths[li] = d[li];
        total_blocks += d[li];
    }
    max_convs = 1 + 3 * total_blocks + 4;
    m->params = (rn_param *)calloc((size_t)max_convs * 5 + 2, sizeof(rn_param));
    m->convs = (rn_conv *)calloc((size_t)max_convs, sizeof(rn_conv));
    m->blocks = (rn_block *)calloc((size_t)total_blocks, sizeof(rn_block));
    m->cap_calls = max_convs;
    m->calls = (rn_conv_call *)calloc((size_t)m->cap_calls, sizeof(rn_conv_call));
    m->share = (struct rn_model_share *)calloc(1, sizeof(struct rn_model_share));
    if (m->share) m->share->model_alive = 1;
    if (!m->params || !m->convs || !m->blocks || !m->calls || !m->share) {
        rn_model_destroy(m);
        return RN_ERR_NOMEM;
    }
    /* stem: conv1 7x7 s2 p3 + bn1 (main.cu:111-112) */
    add_conv(m, "conv1", "bn1", 3, RN_STEM_WIDTH, 7, 2, 3);
    set_geometry(m, RN_DEFAULT_SIDE, RN_DEFAULT_SIDE);
    for (li = 0; li < 4; ++li) {
        for (bi = 0; bi < d[li]; ++bi) {
            rn_block *b = &m->blocks[m->n_blocks++];
            char pre[RN_MAX_KEY], name[RN_MAX_KEY + 16], bn[RN_MAX_KEY + 16];
            const uint64_t stride = bi == 0 ? kStrides[li] : 1;
            uint64_t cin, mid, cout;
            if (m->basic) {
                cout = mid = kBasicWidths[li];
                cin = bi == 0 && li > 0 ? kBasicWidths[li - 1] : cout;
            } else {
                cin = bi == 0 ? kWidths[li][0] : kWidths[li][2];
                mid = mid_width(m, li);
                cout = kWidths[li][2];
            }
            snprintf(pre, sizeof(pre), "layer%d.%d", li + 1, bi);
            snprintf(b->name, RN_MAX_KEY, "%s", pre);
            b->ds = -1;
            b->conv3 = -1;
            /* projection shortcut iff block 0 and (stride != 1 or cin != cout): main.cu:71 */
            if (bi == 0 && (stride != 1 || cin != cout)) {
                snprintf(name, sizeof(name), "%s.downsample.0", pre);
                snprintf(bn, sizeof(bn), "%s.downsample.1", pre);
                b->ds = add_conv(m, name, bn, cin, cout, 1, stride, 0);
            }
            if (m->basic) {
                /* torchvision BasicBlock: conv1 3x3 / stride / pad 1, conv2 3x3 / 1 / 1 */
                snprintf(name, sizeof(name), "%s.conv1", pre);
                snprintf(bn, sizeof(bn), "%s.bn1", pre);
                b->conv1 = add_conv(m, name, bn, cin, cout, 3, stride, 1);
                snprintf(name, sizeof(name), "%s.conv2", pre);
                snprintf(bn, sizeof(bn), "%s.bn2", pre);
                b->conv2 = b->tail = add_conv(m, name, bn, cout, cout, 3, 1, 1);
                continue;
            }
            snprintf(name, sizeof(name), "%s.conv1", pre);
            snprintf(bn, sizeof(bn), "%s.bn1", pre);
            b->conv1 = add_conv(m, name, bn, cin, mid, 1, 1, 0);
            snprintf(name, sizeof(name), "%s.conv2", pre);
            snprintf(bn, sizeof(bn), "%s.bn2", pre);
            b->conv2 = add_conv_grouped(m, name, bn, mid, mid, 3, stride, 1, (uint64_t)groups); /* stride on the 3x3 */
            snprintf(name, sizeof(name), "%s.conv3", pre);
            snprintf(bn, sizeof(bn), "%s.bn3", pre);
            b->conv3 = b->tail = add_conv(m, name, bn, mid, cout, 1, 1, 0);
        }
    }
    m->classes = RN_DEFAULT_CLASSES;
    m->fc_w = add_param(m, "fc.weight", m->classes * m->feat);
    m->fc_b = add_param(m, "fc.bias", m->classes);
    *out = m;
    return RN_OK;
}

int rn_model_create(rn_ctx *ctx, rn_model **out, int arch) { return model_create(ctx, out, arch, 1, 64); }

/* torchvision's bottleneck family: (1, 64) ResNet, (32, 4) / (32, 8) / (64, 4) ResNeXt, (1, 128) Wide ResNet */
int rn_model_create_ex(rn_ctx *ctx, rn_model **out, int depth, int groups, int width_per_group)
{
    const int ok = (groups == 1 && (width_per_group == 64 || width_per_group == 128)) ||
                   (groups == 32 && (width_per_group == 4 || width_per_group == 8)) ||
                   (groups == 64 && width_per_group == 4);
    if (out) *out = NULL;
    if (!ctx || !out) return RN_ERR_INVALID;
    if (!ok || (depth != 50 && depth != 101 && depth != 152)) return RN_ERR_UNSUPPORTED;
    return model_create(ctx, out, depth, groups, width_per_group);
}

int rn_model_set_classes(rn_model *m, uint64_t classes)
{
    if (!m || m->classes_locked || classes < 1 || classes > RN_MAX_CLASSES) return RN_ERR_INVALID;
    m->classes = classes;
    m->params[m->fc_w].numel = classes * m->feat;
    m->params[m->fc_b].numel = classes;
    return RN_OK;
}

uint64_t rn_model_classes(const rn_model *m) { return m ? m->classes : 0; }
uint64_t rn_model_features(const rn_model *m) { return m ? m->feat : 0; }

static void free_acts(rn_model *m)
{
    float **bufs[7];
    int i;
    bufs[0] = &m->x4; bufs[1] = &m->p0; bufs[2] = &m->p1; bufs[3] = &m->dsb;
    bufs[4] = &m->t1; bufs[5] = &m->t2; bufs[6] = &m->pooled;
    for (i = 0; i < 7; ++i) {
        if (*bufs[i]) rn_free(m->ctx, *bufs[i]);
        *bufs[i] = NULL;
    }
    m->batch_cap = 0;
    m->act_bytes = 0;
}

/* The weights do not depend on the image size, the arenas, the tuned tiles and the sub-batch do. */
int rn_model_set_input_size(rn_model *m, uint64_t H, uint64_t W)
{
    rn_model probe;
    int c;
    if (!m || H < RN_MIN_SIDE || H > RN_MAX_SIDE || W < RN_MIN_SIDE || W > RN_MAX_SIDE) return RN_ERR_INVALID;
    /* a captured graph points into the arenas; a pipeline's staging and device buffers hold images of the
     * size it was created at */
    if (m->graphs_live > 0 || m->share->pipelines > 0) return RN_ERR_INVALID;
    probe = *m; /* the geometry of the new size, before anything changes */
    set_geometry(&probe, H, W);
    if (probe.max_sub < 1) return RN_ERR_INVALID;
    if (H == m->H && W == m->W) return RN_OK;
    if (m->batch_cap > 0) { /* forwards still queued read the arenas */
        rn_sync(m->ctx);
        for (c = 0; c < RN_MAX_STREAMS - 1; ++c)
            if (m->ctxn[c]) rn_sync(m->ctxn[c]);
        free_acts(m);
    }
    set_geometry(m, H, W);
    for (c = 0; c < m->n_convs; ++c) {
        m->convs[c].tile[0] = m->convs[c].tile[1] = 0;
        m->convs[c].tile_B[0] = m->convs[c].tile_B[1] = 0;
    }
    for (c = 0; c < m->n_blocks; ++c) {
        m->blocks[c].pair_tile[0] = m->blocks[c].pair_tile[1] = 0;
        m->blocks[c].pair_tile_B[0] = m->blocks[c].pair_tile_B[1] = 0;
    }
    m->tuned_B = 0;
    return RN_OK;
}

/* torchvision's replace_stride_with_dilation: like the input size a property of the model that the weights do
 * not depend on; the arenas, the tuned tiles and the sub-batch do. */
int rn_model_set_dilation(rn_model *m, int layer2, int layer3, int layer4)
{
    rn_model probe;
    int c;
    if (!m || (layer2 | layer3 | layer4) < 0 || layer2 > 1 || layer3 > 1 || layer4 > 1) return RN_ERR_INVALID;
    if (m->basic)
        return rn_ctx_set_error(m->ctx, RN_ERR_UNSUPPORTED,
                                "rn_model_set_dilation: replace_stride_with_dilation is defined for bottleneck "
                                "networks only (torchvision's BasicBlock raises NotImplementedError)");
    /* a captured graph points into the arenas; a pipeline's device buffers are sized by the model */
    if (m->graphs_live > 0 || m->share->pipelines > 0) return RN_ERR_INVALID;
    if (layer2 == m->dilate[0] && layer3 == m->dilate[1] && layer4 == m->dilate[2]) return RN_OK;
    probe = *m; /* the geometry under the new flags, before anything changes */
    probe.dilate[0] = layer2; probe.dilate[1] = layer3; probe.dilate[2] = layer4;
    set_geometry(&probe, m->H, m->W);
    if (probe.max_sub < 1) return RN_ERR_INVALID;
    if (m->batch_cap > 0) { /* forwards still queued read the arenas */
        rn_sync(m->ctx);
        for (c = 0; c < RN_MAX_STREAMS - 1; ++c)
            if (m->ctxn[c]) rn_sync(m->ctxn[c]);
        free_acts(m);
    }
    m->dilate[0] = layer2; m->dilate[1] = layer3; m->dilate[2] = layer4;
    apply_dilation(m);
    set_geometry(m, m->H, m->W);
    for (c = 0; c < m->n_convs; ++c) {
        m->convs[c].tile[0] = m->convs[c].tile[1] = 0;
        m->convs[c].tile_B[0] = m->convs[c].tile_B[1] = 0;
    }
    for (c = 0; c < m->n_blocks; ++c) {
        m->blocks[c].pair_tile[0] = m->blocks[c].pair_tile[1] = 0;
        m->blocks[c].pair_tile_B[0] = m->blocks[c].pair_tile_B[1] = 0;
    }
    m->tuned_B = 0;
    return RN_OK;
}

int rn_model_dilation(const rn_model *m, int out[3])
{
    if (!m || !out) return RN_ERR_INVALID;
    out[0] = m->dilate[0]; out[1] = m->dilate[1]; out[2] = m->dilate[2];
    return RN_OK;
}

/* input pixels per pixel of the final map: 32, or 16 / 8 / 4 with one / two / three dilated stages */
int rn_model_output_stride(const rn_model *m)
{
    return m ? 32 >> (m->dilate[0] + m->dilate[1] + m->dilate[2]) : 0;
}

int rn_model_input_size(const rn_model *m, uint64_t *H, uint64_t *W)
{
    if (!m) return RN_ERR_INVALID;
    if (H) *H = m->H;
    if (W) *W = m->W;
    return RN_OK;
}

uint64_t rn_model_max_sub_batch(const rn_model *m) { return m ? m->max_sub : 0; }

/* the map behind stage 1..4: the stage's stride (1 where it is dilated) on the map before it, as set_geometry */
int rn_model_stage_shape(const rn_model *m, int stage, uint64_t *C, uint64_t *H, uint64_t *W)
{
    uint64_t h, w;
    int li;
    if (!m || stage < 1 || stage > 4) return RN_ERR_INVALID;
    h = m->pool_h;
    w = m->pool_w;
    for (li = 0; li < stage; ++li) {
        const uint64_t stride = li > 0 && m->dilate[li - 1] ? 1 : kStrides[li];
        h = rn_conv_output_size(h, 1, stride, 0);
        w = rn_conv_output_size(w, 1, stride, 0);
    }
    if (C) *C = m->basic ? kBasicWidths[stage - 1] : kWidths[stage - 1][2];
    if (H) *H = h;
    if (W) *W = w;
    return RN_OK;
}

static void free_prof(rn_model *m)
{
    uint64_t i;
    for (i = 0; i < m->cap_prof; ++i) {
        rn_event_destroy(m->prof[i].start);
        rn_event_destroy(m->prof[i].stop);
    }
    free(m->prof);
    m->prof = NULL;
    m->n_prof = m->cap_prof = 0;
}

int rn_model_destroy(rn_model *m)
{
    uint64_t i;
    int c;
    if (!m) return RN_OK;
    /* a captured graph points into this model's arenas, weights and the scratch of the contexts of
     * its extra streams, and rn_graph_destroy unpins those contexts: the graphs go first */
    if (m->graphs_live > 0) return RN_ERR_INVALID;
    if (m->ctx) rn_sync(m->ctx);
    if (m->share) {
        m->share->model_alive = 0;
        if (m->share->pipelines == 0) free(m->share);
    }
    if (m->params) {
        for (i = 0; i < m->n_params; ++i) rn_free(m->ctx, m->params[i].dev);
    }
    if (m->convs) {
        for (c = 0; c < m->n_convs; ++c) {
            rn_free(m->ctx, m->convs[c].packed);
            rn_free(m->ctx, m->convs[c].scale);
            rn_free(m->ctx, m->convs[c].shift);
        }
    }
    if (m->blocks) {
        for (c = 0; c < m->n_blocks; ++c) {
            rn_free(m->ctx, m->blocks[c].pair_packed);
            rn_free(m->ctx, m->blocks[c].pair_shift);
        }
    }
    rn_free(m->ctx, m->fc_packed);
    rn_free(m->ctx, m->stem_packed_exact);
    rn_free(m->ctx, m->stem_pool_packed);
    if (m->crops) rn_free(m->ctx, m->crops);
    if (m->own_logits) rn_free(m->ctx, m->own_logits);
    free_acts(m);
    free_prof(m);
    {
        int k;
        rn_event_destroy(m->ev_fork);
        for (k = 0; k < RN_MAX_STREAMS - 1; ++k) {
            if (!m->ctxn[k]) continue;
            rn_sync(m->ctxn[k]);
            rn_event_destroy(m->ev_join[k]);
            rn_ctx_destroy(m->ctxn[k]);
        }
    }
    free(m->params);
    free(m->convs);
    free(m->blocks);
    free(m->calls);
    free(m);
    return RN_OK;
}

const char *rn_model_tensor_key(const rn_model *m, uint64_t index, uint64_t *numel)
{
    if (!m || index >= m->n_params) return NULL;
    if (numel) *numel = m->params[index].numel;
    return m->params[index].key;
}

int rn_model_set_tensor(rn_model *m, const char *key, const float *host_data, uint64_t numel)
{
    uint64_t i;
    if (!m || !key || !host_data) return RN_ERR_INVALID;
    for (i = 0; i < m->n_params; ++i) {
        rn_param *p = &m->params[i];
        if (strcmp(p->key, key) != 0) continue;
        if (p->numel != numel) return RN_ERR_INVALID;
        m->classes_locked = 1;
        if (!p->dev) {
            int st = rn_malloc(m->ctx, (void **)&p->dev, numel * sizeof(float));
            if (st != RN_OK) return st;
        }
        p->is_set = 1;
        m->finalized = 0;
        return rn_memcpy_h2d(m->ctx, p->dev, host_data, numel * sizeof(float));
    }
    return RN_ERR_INVALID; /* unknown key (e.g. *.num_batches_tracked): callers skip those */
}

int rn_model_load_dir(rn_model *m, const char *weights_dir)
{
    uint64_t i;
    if (!m || !weights_dir) return RN_ERR_INVALID;
    m->classes_locked = 1;
    for (i = 0; i < m->n_params; ++i) {
        rn_param *p = &m->params[i];
        char path[1024];
        float *dev = NULL;
        uint64_t n = 0;
        int st;
        snprintf(path, sizeof(path), "%s/%s", weights_dir, p->key);
        st = rn_load_f32_file(m->ctx, path, &dev, &n);
        if (st != RN_OK) return st;
        if (n != p->numel) {
            rn_free(m->ctx, dev);
            return RN_ERR_INVALID;
        }
        if (p->dev) rn_free(m->ctx, p->dev);
        p->dev = dev;
        p->is_set = 1;
    }
    m->finalized = 0;
    return RN_OK;
}

static uint64_t elem_size(const rn_model *m) { return m->dtype == RN_DTYPE_BF16 ? 2 : 4; }

int rn_model_set_dtype(rn_model *m, int dtype)
{
    int c;
    if (!m || (dtype != RN_DTYPE_F32 && dtype != RN_DTYPE_BF16)) return RN_ERR_INVALID;
    if (!m->streams_set) m->streams = 2; /* measured default for both element types (fp32 +0.8 %, bf16 +5 %) */
    if (dtype == m->dtype) return RN_OK;
    /* packed panels and arenas depend on the element size: drop them */
    for (c = 0; c < m->n_convs; ++c) {
        rn_free(m->ctx, m->convs[c].packed);
        m->convs[c].packed = NULL;
        m->convs[c].tile[0] = m->convs[c].tile[1] = 0;
    }
    for (c = 0; c < m->n_blocks; ++c) {
        rn_free(m->ctx, m->blocks[c].pair_packed);
        m->blocks[c].pair_packed = NULL;
        m->blocks[c].pair_tile[0] = m->blocks[c].pair_tile[1] = 0;
    }
    rn_free(m->ctx, m->fc_packed);
    m->fc_packed = NULL;
    rn_free(m->ctx, m->stem_pool_packed);
    m->stem_pool_packed = NULL;
    free_acts(m);
    m->dtype = dtype;
    m->finalized = 0;
    m->tuned_B = 0;
    return RN_OK;
}

int rn_model_finalize(rn_model *m)
{
    uint64_t i;
    int c, st;
    if (!m) return RN_ERR_INVALID;
    m->classes_locked = 1;
    for (i = 0; i < m->n_params; ++i) {
        if (!m->params[i].is_set) return RN_ERR_INVALID;
    }
    /* the bf16 classifier is the bf16 contraction, which refuses logits rows off a 16-byte boundary: those
     * of the later parts of a batch when the class count is no multiple of 4 */
    if (m->dtype != RN_DTYPE_F32 && m->classes % 4 != 0) return RN_ERR_UNSUPPORTED;
    for (c = 0; c < m->n_convs; ++c) {
        rn_conv *cv = &m->convs[c];
        const uint64_t pn = cv->groups > 1 ? rn_conv2d_grouped_packed_weight_numel_dt(m->dtype, cv->cin, cv->cout,
                                                                                     cv->k, cv->groups)
                                           : rn_conv2d_packed_weight_numel_dt(m->dtype, cv->cin, cv->cout, cv->k);
        if (!cv->packed) {
            st = rn_malloc(m->ctx, &cv->packed, pn * elem_size(m));
            if (st != RN_OK) return st;
        }
        if (!cv->scale) {
            st = rn_malloc(m->ctx, (void **)&cv->scale, cv->cout * sizeof(float));
            if (st != RN_OK) return st;
            st = rn_malloc(m->ctx, (void **)&cv->shift, cv->cout * sizeof(float));
            if (st != RN_OK) return st;
        }
        st = cv->groups > 1 ? rn_conv2d_grouped_pack_weight_dt(m->ctx, m->dtype, m->params[cv->w].dev, cv->packed,
                                                               cv->cin, cv->cout, cv->k, cv->groups)
                            : rn_conv2d_pack_weight_dt(m->ctx, m->dtype, m->params[cv->w].dev, cv->packed, cv->cin,
                                                       cv->cout, cv->k);
        if (st != RN_OK) return st;
        st = rn_batchnorm2d_fold(m->ctx, m->params[cv->bn_w].dev, m->params[cv->bn_b].dev,
                                 m->params[cv->bn_m].dev, m->params[cv->bn_v].dev, cv->scale,
                                 cv->shift, cv->cout);
        if (st != RN_OK) return st;
    }
    if (m->dtype == RN_DTYPE_F32) {
        const rn_conv *stem = &m->convs[0];
        if (!m->stem_packed_exact) {
            st = rn_malloc(m->ctx, (void **)&m->stem_packed_exact,
                           rn_conv2d_packed_weight_numel_exact(stem->cin, stem->cout, stem->k) *
                               sizeof(float));
            if (st != RN_OK) return st;
        }
        st = rn_conv2d_pack_weight_exact(m->ctx, m->params[stem->w].dev, m->stem_packed_exact,
                                         stem->cin, stem->cout, stem->k);
        if (st != RN_OK) return st;
    }
    {   /* panel of the fused stem + max-pool launch */
        const rn_conv *stem = &m->convs[0];
        if (!m->stem_pool_packed) {
            st = rn_malloc(m->ctx, &m->stem_pool_packed, rn_stem_pool_packed_weight_numel(m->dtype) * elem_size(m));
            if (st != RN_OK) return st;
        }
        st = rn_stem_pool_pack_weight_dt(m->ctx, m->dtype, m->params[stem->w].dev, m->stem_pool_packed, stem->cin);
        if (st != RN_OK) return st;
    }
    for (c = 0; c < m->n_blocks; ++c) {
        rn_block *b = &m->blocks[c];
        const rn_conv *c3, *cd;
        if (b->ds < 0) continue;
        c3 = &m->convs[b->tail];
        cd = &m->convs[b->ds];
        if (!b->pair_packed) {
            st = rn_malloc(m->ctx, &b->pair_packed,
                           rn_conv2d_packed_pair_weight_numel(c3->cin, c3->cout, c3->k, cd->cin) *
                               elem_size(m));
            if (st != RN_OK) return st;
        }
        if (!b->pair_shift) {
            st = rn_malloc(m->ctx, (void **)&b->pair_shift, c3->cout * sizeof(float));
            if (st != RN_OK) return st;
        }
        st = rn_conv2d_pack_weight_pair_dt(m->ctx, m->dtype, m->params[c3->w].dev, c3->scale,
                                           m->params[cd->w].dev, cd->scale, b->pair_packed, c3->cin,
                                           c3->cout, c3->k, cd->cin);
        if (st != RN_OK) return st;
        st = rn_add_forward(m->ctx, c3->shift, cd->shift, b->pair_shift, c3->cout);
        if (st != RN_OK) return st;
    }
    if (m->dtype != RN_DTYPE_F32) {
        /* fc.weight [classes][feat] is a 1x1 convolution panel: same packer, k = 1 */
        if (!m->fc_packed) {
            st = rn_malloc(m->ctx, &m->fc_packed, m->classes * m->feat * elem_size(m));
            if (st != RN_OK) return st;
        }
        st = rn_conv2d_pack_weight_dt(m->ctx, m->dtype, m->params[m->fc_w].dev, m->fc_packed, m->feat,
                                      m->classes, 1);
        if (st != RN_OK) return st;
    }
    st = rn_sync(m->ctx);
    if (st != RN_OK) return st;
    m->finalized = 1;
    return RN_OK;
}

static int ensure_acts(rn_model *m, uint64_t B)
{
    int st;
    if (B <= m->batch_cap) return RN_OK;
    if (m->batch_cap > 0 && rn_ctx_graphs_live(m->ctx) > 0)
        return RN_ERR_INVALID; /* captured graphs point into the arenas: destroy them first */
    free_acts(m);
    {
        const uint64_t es = elem_size(m);
        st = rn_malloc(m->ctx, (void **)&m->x4, B * m->x4_img * es);
        if (st == RN_OK) st = rn_malloc(m->ctx, (void **)&m->p0, B * m->p_img * es);
        if (st == RN_OK) st = rn_malloc(m->ctx, (void **)&m->p1, B * m->p_img * es);
        if (st == RN_OK) st = rn_malloc(m->ctx, (void **)&m->dsb, B * m->ds_img * es);
        if (st == RN_OK) st = rn_malloc(m->ctx, (void **)&m->t1, B * m->t1_img * es);
        if (st == RN_OK && m->t2_img) st = rn_malloc(m->ctx, (void **)&m->t2, B * m->t2_img * es);
        if (st == RN_OK) st = rn_malloc(m->ctx, (void **)&m->pooled, B * m->feat * es);
    }
    if (st != RN_OK) {
        free_acts(m);
        return st;
    }
    m->batch_cap = B;
    m->act_bytes = B * (m->x4_img + 2 * m->p_img + m->ds_img + m->t1_img + m->t2_img + m->feat) * elem_size(m);
    return RN_OK;
}

uint64_t rn_model_activation_bytes(const rn_model *m) { return m ? m->act_bytes : 0; }

/* library-internal: the pipeline (rn_pipeline.hip) queues on the model's stream */
rn_ctx *rn_model_context(rn_model *m) { return m ? m->ctx : NULL; }

/* library-internal: every context the model has queued batch parts on (m->ctx and the m->ctxn[]
 * of the other streams).  A captured forward holds pointers into the scratch of each of them:
 * rn_model_capture pins them all for the graph's lifetime (rn_scratch refuses to grow a pinned
 * context's slots). */
int rn_model_contexts(rn_model *m, rn_ctx **out, int cap)
{
    int k, n = 0;
    if (!m || !out) return 0;
    if (n < cap) out[n++] = m->ctx;
    for (k = 0; k < RN_MAX_STREAMS - 1; ++k)
        if (m->ctxn[k] && n < cap) out[n++] = m->ctxn[k];
    return n;
}
/* library-internal: the pipelines of this model (see rn_private.h) */
void *rn_model_pipeline_attach(rn_model *m)
{
    if (!m) return NULL;
    ++m->share->pipelines;
    return m->share;
}

void rn_model_pipeline_detach(void *cell)
{
    struct rn_model_share *sh = (struct rn_model_share *)cell;
    if (!sh) return;
    --sh->pipelines;
    if (!sh->model_alive && sh->pipelines == 0) free(sh);
}

/* library-internal: rn_model_capture / rn_graph_destroy count the graphs that hold this model */
void rn_model_graph_ref(rn_model *m, int delta)
{
    if (m) m->graphs_live += delta;
}

int rn_model_set_pair_fusion(rn_model *m, int on)
{
    if (!m) return RN_ERR_INVALID;
    m->pair_fusion = on ? 1 : 0;
    m->tuned_B = 0; /* the set of launches changes */
    return RN_OK;
}

int rn_model_set_streams(rn_model *m, int streams)
{
    if (!m || (streams != 0 && streams != 1 && streams != 2 && streams != 4)) return RN_ERR_INVALID;
    if (streams == 0) { /* back to the library default, as if this function had never been called */
        m->streams = 2;
        m->streams_set = 0;
        return RN_OK;
    }
    m->streams = streams;
    m->streams_set = 1;
    /* the tuned tiles are looked up by launch batch size: those of other part sizes simply stop matching */
    return RN_OK;
}

int rn_model_get_streams(const rn_model *m) { return m ? m->streams : 0; }

static int parts_of(const rn_model *m, uint64_t B);
int rn_model_parts(const rn_model *m, uint64_t B) { return m && B ? parts_of(m, B) : 0; }

int rn_model_set_stem_pool_fusion(rn_model *m, int on)
{
    if (!m) return RN_ERR_INVALID;
    m->stem_pool = on < 0 ? 0 : on > 2 ? 2 : on; /* 2: fetch the patches from the NCHW input */
    m->tuned_B = 0;
    return RN_OK;
}

int rn_model_set_chain(rn_model *m, int on)
{
    if (!m) return RN_ERR_INVALID;
    m->chain = on ? 1 : 0;
    return RN_OK;
}

int rn_model_set_front_parts(rn_model *m, int parts)
{
    if (!m || parts < 1 || parts > 16 || (parts & (parts - 1))) return RN_ERR_INVALID;
    m->front_parts = parts;
    m->tuned_B = 0;
    return RN_OK;
}

int rn_model_set_stem_exact(rn_model *m, int on)
{
    if (!m) return RN_ERR_INVALID;
    m->stem_exact = on ? 1 : 0;
    m->tuned_B = 0;
    return RN_OK;
}

int rn_model_profiling_enabled(const rn_model *m) { return m ? m->profiling : 0; }

/* ---- profiling --------------------------------------------------------- */
static int prof_begin(rn_model *m, const char *op, const char *layer, double flops, double bytes)
{
    rn_prof *r;
    if (!m->profiling) return RN_OK;
    if (m->n_prof == m->cap_prof) {
        const uint64_t ncap = m->cap_prof ? m->cap_prof * 2 : 256;
        rn_prof *np = (rn_prof *)realloc(m->prof, ncap * sizeof(rn_prof));
        uint64_t i;
        if (!np) return RN_ERR_NOMEM;
        m->prof = np;
        for (i = m->cap_prof; i < ncap; ++i) {
            int st;
            memset(&np[i], 0, sizeof(rn_prof));
            st = rn_event_create(m->run.ctx, &np[i].start);
            if (st == RN_OK) st = rn_event_create(m->run.ctx, &np[i].stop);
            if (st != RN_OK) {
                m->cap_prof = i;
                return st;
            }
        }
        m->cap_prof = ncap;
    }
    r = &m->prof[m->n_prof];
    r->op = op;
    snprintf(r->layer, RN_MAX_KEY, "%s", layer);
    r->flops = flops;
    r->bytes = bytes;
    r->ms = -1.f;
    return rn_event_record(m->run.ctx, r->start);
}

static int prof_end(rn_model *m)
{
    if (!m->profiling) return RN_OK;
    return rn_event_record(m->run.ctx, m->prof[m->n_prof++].stop);
}

int rn_model_set_profiling(rn_model *m, int on)
{
    if (!m) return RN_ERR_INVALID;
    m->profiling = on ? 1 : 0;
    return RN_OK;
}

uint64_t rn_model_profile_count(const rn_model *m) { return m ? m->n_prof : 0; }

int rn_model_profile_get(const rn_model *m, uint64_t index, const char **op_name,
                         const char **layer_name, float *ms, double *flops, double *bytes)
{
    rn_prof *r;
    if (!m || index >= m->n_prof) return RN_ERR_INVALID;
    r = &m->prof[index];
    if (r->ms < 0.f) {
        int st = rn_event_elapsed_ms(r->start, r->stop, &r->ms);
        if (st != RN_OK) return st;
    }
    if (op_name) *op_name = r->op;
    if (layer_name) *layer_name = r->layer;
    if (ms) *ms = r->ms;
    if (flops) *flops = r->flops;
    if (bytes) *bytes = r->bytes;
    return RN_OK;
}

#define TRY(expr)                   \
    do {                            \
        int st_ = (expr);           \
        if (st_ != RN_OK) return st_; \
    } while (0)

/* ---- ops with profiling brackets --------------------------------------- */
/* next record of the tuning pass's call list (the slices of a depth-first front repeat calls) */
static rn_conv_call *next_call(rn_model *m)
{
    if (m->n_calls == m->cap_calls) {
        const int ncap = 2 * m->cap_calls + 16;
        rn_conv_call *nc = (rn_conv_call *)realloc(m->calls, (size_t)ncap * sizeof(rn_conv_call));
        if (!nc) return NULL;
        m->calls = nc;
        m->cap_calls = ncap;
    }
    return &m->calls[m->n_calls++];
}

/* the tile tuned for a launch of B images in the current mode, or 0 = per-launch choice */
static int tuned_tile(const rn_model *m, const int tile[2], const uint64_t tile_B[2], uint64_t B)
{
    if (!m->tuned_B || m->tuned_mode != m->run.mode) return 0;
    return tile_B[0] == B ? tile[0] : tile_B[1] == B ? tile[1] : 0;
}

/* the one place a contraction is launched: the exact-K stem, the fused pair, the grouped or the dense kernel */
static int launch_call(const rn_model *m, rn_ctx *ctx, const rn_conv_call *k)
{
    const rn_conv *cv = &m->convs[k->conv];
    const rn_epilogue *ep = k->has_ep ? &k->ep : NULL;
    const uint64_t ho = conv_side(cv, k->H, k->pad), wo = conv_side(cv, k->W, k->pad);
    if (k->pair_block >= 0) {
        const rn_block *pb = &m->blocks[k->pair_block];
        const rn_conv *cd = &m->convs[pb->ds];
        rn_conv_second second;
        second.inp = k->x2; second.in_channels = cd->cin; second.H = k->H2; second.W = k->W2;
        second.stride = cd->stride;
        return rn_conv2d_nhwc_pair_forward_dt(ctx, m->dtype, m->dtype, k->x, k->y, pb->pair_packed, cv->k,
                                              cv->stride, k->pad, ho, wo, k->B, cv->cin, cv->cout, k->H, k->W,
                                              &second, ep);
    }
    if (k->exact)
        return rn_conv2d_nhwc_exact_forward(ctx, (const float *)k->x, (float *)k->y, m->stem_packed_exact, cv->k,
                                            cv->stride, ho, wo, k->B, cv->cin, cv->cout, k->H, k->W, ep);
    if (cv->dil > 1) /* conv2 of a dilated stage, dense or grouped: the same panel, the taps dil apart */
        return rn_conv2d_dilated_nhwc_forward_dt(ctx, m->dtype, m->dtype, k->x, k->y, cv->packed, cv->k, cv->stride,
                                                 k->pad, cv->dil, ho, wo, k->B, cv->cin, cv->cout, k->H, k->W,
                                                 cv->groups, ep);
    if (cv->groups > 1) /* one kernel, no tile candidates: every candidate times the same launch */
        return rn_conv2d_grouped_nhwc_forward_dt(ctx, m->dtype, m->dtype, k->x, k->y, cv->packed, cv->k, cv->stride,
                                                 k->pad, ho, wo, k->B, cv->cin, cv->cout, k->H, k->W, cv->groups, ep);
    return rn_conv2d_nhwc_forward_dt(ctx, m->dtype, m->dtype, k->x, k->y, cv->packed, cv->k, cv->stride, k->pad, ho,
                                     wo, k->B, cv->cin, cv->cout, k->H, k->W, ep);
}

/* a contraction of the forward being queued: on the call list when recording, then inside its profile
 * bracket and with its tuned tile through launch_call */
static int op_call(rn_model *m, const rn_conv_call *k, const char *op, const char *layer, double flops,
                   double bytes, const int tile[2], const uint64_t tile_B[2])
{
    int st;
    if (m->recording) {
        rn_conv_call *c = next_call(m);
        if (!c) return RN_ERR_NOMEM;
        *c = *k;
    }
    TRY(prof_begin(m, op, layer, flops, bytes));
    rn_ctx_set_conv_tile(m->run.ctx, tuned_tile(m, tile, tile_B, k->B));
    st = launch_call(m, m->run.ctx, k);
    rn_ctx_set_conv_tile(m->run.ctx, 0);
    if (st != RN_OK) return st;
    return prof_end(m);
}

/* x [B,H,W,cin] -> y.  pad replaces the layer's padding where the image carries its own zero border
 * (H, W are then the padded sizes and pad is 0); exact: the fp32 stem in its exact-K form */
static int op_conv_at(rn_model *m, const rn_conv *cv, const void *x, void *y, uint64_t B, uint64_t H,
                      uint64_t W, const rn_epilogue *ep, uint64_t pad, int exact)
{
    const uint64_t ho = conv_side(cv, H, pad), wo = conv_side(cv, W, pad);
    /* a grouped convolution counts its algorithmic products: K = k*k*cin/groups per output */
    const double M = (double)(B * ho * wo), K = (double)(cv->cin / cv->groups * cv->k * cv->k);
    const double es = (double)elem_size(m);
    double bytes = es * ((double)(B * H * W * cv->cin) + K * (double)cv->cout +
                         M * (double)cv->cout);
    rn_conv_call k;
    if (ep && ep->residual) bytes += es * M * (double)cv->cout;
    memset(&k, 0, sizeof(k));
    k.conv = (int)(cv - m->convs);
    k.pair_block = -1;
    k.exact = exact;
    k.x = x; k.y = y;
    k.B = B; k.H = H; k.W = W; k.pad = pad;
    k.has_ep = ep != NULL;
    if (ep) k.ep = *ep;
    return op_call(m, &k, ep ? "conv2d+epilogue" : "conv2d", cv->name, 2.0 * M * (double)cv->cout * K, bytes,
                   cv->tile, cv->tile_B);
}

static int op_conv(rn_model *m, const rn_conv *cv, const void *x, void *y, uint64_t B, uint64_t H,
                   uint64_t W, const rn_epilogue *ep)
{
    return op_conv_at(m, cv, x, y, B, H, W, ep, cv->pad, 0);
}

/* conv3 (input t, [B,H,W,c3->cin]) + downsample (input x, [B,H2,W2,cd->cin]) + shifts + ReLU; in a
 * basic block conv2 (3x3 / 1 / 1, same H x W in and out) takes conv3's place */
static int op_pair(rn_model *m, rn_block *b, const void *t, const void *x, void *y, uint64_t B,
                   uint64_t H, uint64_t W, uint64_t H2, uint64_t W2)
{
    const rn_conv *c3 = &m->convs[b->tail], *cd = &m->convs[b->ds];
    const double M = (double)(B * H * W), K = (double)(c3->cin * c3->k * c3->k + cd->cin);
    const double es = (double)elem_size(m);
    const double bytes = es * ((double)(B * H * W * c3->cin) + (double)(B * H2 * W2 * cd->cin) +
                               K * (double)c3->cout + M * (double)c3->cout);
    char name[RN_MAX_KEY];
    rn_conv_call k;
    memset(&k, 0, sizeof(k));
    k.conv = b->tail;
    k.pair_block = (int)(b - m->blocks);
    k.x = t; k.x2 = x; k.y = y;
    k.B = B; k.H = H; k.W = W; k.pad = c3->pad; k.H2 = H2; k.W2 = W2;
    k.has_ep = 1;
    k.ep.scale = NULL; k.ep.shift = b->pair_shift; k.ep.residual = NULL; k.ep.relu = 1;
    snprintf(name, sizeof(name), "%.*s+downsample", (int)(RN_MAX_KEY - 12), c3->name);
    return op_call(m, &k, "conv2d+epilogue", name, 2.0 * M * (double)c3->cout * K, bytes, b->pair_tile,
                   b->pair_tile_B);
}

/* conv3 + bn3 + residual + ReLU of block b and conv1 + bn1 + ReLU of the block after it as one
 * launch (rn_conv_chain_forward_dt): t2 -> y (written: the next block's residual) -> the next
 * block's t1, y reaching conv1 through LDS.  Algorithmic work: both contractions' FLOPs; bytes
 * t2 + residual + y + t1 + both weight panels (y is not read back). */
static int chain_applies(const rn_model *m, const rn_block *b, int mode)
{
    const int bi = (int)(b - m->blocks);
    const rn_conv *c3, *n1;
    if (m->basic) return 0; /* chains are 1x1 -> 1x1; a basic block ends in a 3x3 */
    c3 = &m->convs[b->conv3];
    if (!m->chain || mode != RN_FWD_FUSED || m->recording) return 0;
    if (b->ds >= 0) { /* first block of a stage: only as the fused pair at equal resolution (stage 1) */
        const rn_conv *cd = &m->convs[b->ds];
        if (!m->pair_fusion || cd->stride != 1 || cd->cin != 64) return 0;
    }
    if (bi + 1 >= m->n_blocks) return 0;
    if (m->front_parts > 1 && bi + 1 == m->depths[0]) return 0; /* the next block runs in another slice */
    n1 = &m->convs[m->blocks[bi + 1].conv1];
    if (c3->k != 1 || c3->stride != 1 || n1->k != 1 || n1->stride != 1 || n1->cin != c3->cout) return 0;
    if (c3->cin == 64 && c3->cout == 256) return n1->cout == 64 || n1->cout == 128;
    if (m->dtype != RN_DTYPE_BF16 || b->ds >= 0) return 0;
    /* bf16: the 128-channel blocks of stage 2 (panels in registers).  A chain for the 256-channel
     * blocks of stage 3 (panels streamed through LDS) was built in round 3 and measured 112 us against
     * 91-95 for its two launches (profiles/round3/chain_against_two_launches_bf16.txt): removed */
    return c3->cin == 128 && c3->cout == 512 && n1->cout == 128;
}

static int op_chain(rn_model *m, const rn_block *b, const void *t2, const void *shortcut, void *y,
                    uint64_t B, uint64_t H, uint64_t W)
{
    const rn_conv *c3 = &m->convs[b->conv3];
    const rn_conv *n1 = &m->convs[m->blocks[(b - m->blocks) + 1].conv1];
    const double M = (double)(B * H * W), es = (double)elem_size(m);
    char name[RN_MAX_KEY];
    snprintf(name, sizeof(name), "%.*s%s+next.conv1", (int)(RN_MAX_KEY - 24), c3->name, b->ds >= 0 ? "+downsample" : "");
    {
        const double k1 = (double)c3->cin + (b->ds >= 0 ? (double)m->convs[b->ds].cin : 0.0);
        /* second operand of the first product: the residual (c3->cout channels) or the block input */
        const double op2 = b->ds >= 0 ? (double)m->convs[b->ds].cin : (double)c3->cout;
        TRY(prof_begin(m, "conv2d+epilogue+conv2d", name,
                       2.0 * M * ((double)c3->cout * k1 + (double)n1->cout * (double)n1->cin),
                       es * (M * ((double)c3->cin + op2 + (double)c3->cout + (double)n1->cout) +
                             (double)c3->cout * k1 + (double)(n1->cout * n1->cin))));
    }
    if (b->ds >= 0) /* shortcut = the block's input: the downsample branch rides in the first product */
        TRY(rn_conv_chain_pair_forward_dt(m->run.ctx, m->dtype, t2, shortcut, y, b->pair_packed, b->pair_shift,
                                          m->run.t1, n1->packed, n1->scale, n1->shift, B * H * W, c3->cin,
                                          m->convs[b->ds].cin, c3->cout, n1->cout));
    else
        TRY(rn_conv_chain_forward_dt(m->run.ctx, m->dtype, t2, shortcut, y, c3->packed, c3->scale, c3->shift,
                                     m->run.t1, n1->packed, n1->scale, n1->shift, B * H * W, c3->cin,
                                     c3->cout, n1->cout));
    m->run.t1_ready = 1;
    return prof_end(m);
}

static int op_bn(rn_model *m, const rn_conv *cv, float *y, uint64_t B, uint64_t HW)
{
    const double n = (double)(B * cv->cout * HW);
    TRY(prof_begin(m, "batchnorm2d", cv->name, 0.0, 8.0 * n + 16.0 * (double)cv->cout));
    TRY(rn_batchnorm2d_forward(m->run.ctx, y, y, m->params[cv->bn_w].dev, m->params[cv->bn_b].dev,
                               m->params[cv->bn_m].dev, m->params[cv->bn_v].dev, B, cv->cout, HW));
    return prof_end(m);
}

static int op_relu(rn_model *m, const char *layer, float *y, uint64_t n)
{
    TRY(prof_begin(m, "relu", layer, 0.0, 8.0 * (double)n));
    TRY(rn_relu_forward(m->run.ctx, y, y, n));
    return prof_end(m);
}

static int op_add(rn_model *m, const char *layer, float *y, const float *shortcut, uint64_t n)
{
    TRY(prof_begin(m, "add", layer, 0.0, 12.0 * (double)n));
    TRY(rn_add_forward(m->run.ctx, y, shortcut, y, n)); /* out aliases inp1: main.cu:162 */
    return prof_end(m);
}

/* the reference-ops downsample branch: conv + bn into dsb */
static int op_downsample(rn_model *m, const rn_conv *cd, const float *x, uint64_t B, uint64_t h, uint64_t w,
                         uint64_t HWo)
{
    TRY(op_conv(m, cd, x, m->run.dsb, B, h, w, NULL));
    return op_bn(m, cd, m->run.dsb, B, HWo);
}

/* One residual block, x -> y, both NHWC (layerForward body, main.cu:131-164).
 *   bottleneck: conv1 1x1, conv2 3x3 (carries the stride, may be grouped), tail conv3 1x1;
 *   basic (torchvision BasicBlock): conv1 3x3 (carries the stride), no conv2 stage, tail conv2 3x3;
 *   it never chains (chain_applies).
 * Fused: each convolution with its batch-norm and ReLU, the tail with the shortcut.  With pair fusion,
 * a block with a downsample branch runs the tail and that branch as one contraction: the downsample
 * tensor is never materialised, its K rows ride in the tail's loop (one fp32 sum over both K ranges
 * instead of two rounded results added: not bit-neutral).
 * Reference ops: the reference's order; the downsample branch is queued first in a bottleneck block
 * and after conv2 + bn2 in a basic block. */
static int block_forward(rn_model *m, rn_block *b, const float *x, float *y, uint64_t B,
                         uint64_t *H, uint64_t *W, int mode)
{
    const rn_conv *c1 = &m->convs[b->conv1], *ct = &m->convs[b->tail];
    const rn_conv *c2 = m->basic ? NULL : &m->convs[b->conv2]; /* the middle stage */
    const rn_conv *cd = b->ds >= 0 ? &m->convs[b->ds] : NULL;
    const rn_conv *cs = c2 ? c2 : c1;                          /* where the stride sits */
    const uint64_t h = *H, w = *W;
    const uint64_t ho = conv_side(cs, h, cs->pad), wo = conv_side(cs, w, cs->pad);
    const uint64_t h1 = c2 ? h : ho, w1 = c2 ? w : wo;         /* conv1's output */
    float *mid = c2 ? m->run.t2 : m->run.t1;                   /* the tail's input */
    const float *shortcut = x;
    if (mode == RN_FWD_FUSED) {
        rn_epilogue ep;
        const int pair = cd && m->pair_fusion;
        if (cd && !pair) {
            ep.scale = cd->scale; ep.shift = cd->shift; ep.residual = NULL; ep.relu = 0;
            TRY(op_conv(m, cd, x, m->run.dsb, B, h, w, &ep));
            shortcut = m->run.dsb;
        }
        ep.scale = c1->scale; ep.shift = c1->shift; ep.residual = NULL; ep.relu = 1;
        if (m->run.t1_ready)
            m->run.t1_ready = 0; /* the block before has left this conv1's output in t1 (op_chain) */
        else
            TRY(op_conv(m, c1, x, m->run.t1, B, h, w, &ep));
        if (c2) {
            ep.scale = c2->scale; ep.shift = c2->shift;
            TRY(op_conv(m, c2, m->run.t1, m->run.t2, B, h, w, &ep));
        }
        if (chain_applies(m, b, mode)) {
            TRY(op_chain(m, b, mid, pair ? x : shortcut, y, B, ho, wo));
        } else if (pair) {
            TRY(op_pair(m, b, mid, x, y, B, ho, wo, h, w));
        } else {
            ep.scale = ct->scale; ep.shift = ct->shift; ep.residual = shortcut;
            TRY(op_conv(m, ct, mid, y, B, ho, wo, &ep));
        }
    } else {
        if (cd) shortcut = m->run.dsb;
        if (cd && c2) TRY(op_downsample(m, cd, x, B, h, w, ho * wo));
        TRY(op_conv(m, c1, x, m->run.t1, B, h, w, NULL));
        TRY(op_bn(m, c1, m->run.t1, B, h1 * w1));
        TRY(op_relu(m, c1->name, m->run.t1, B * h1 * w1 * c1->cout));
        if (c2) {
            TRY(op_conv(m, c2, m->run.t1, m->run.t2, B, h, w, NULL));
            TRY(op_bn(m, c2, m->run.t2, B, ho * wo));
            TRY(op_relu(m, c2->name, m->run.t2, B * ho * wo * c2->cout));
        }
        TRY(op_conv(m, ct, mid, y, B, ho, wo, NULL));
        TRY(op_bn(m, ct, y, B, ho * wo));
        if (cd && !c2) TRY(op_downsample(m, cd, x, B, h, w, ho * wo));
        TRY(op_add(m, b->name, y, shortcut, B * ho * wo * ct->cout));
        TRY(op_relu(m, b->name, y, B * ho * wo * ct->cout));
    }
    *H = ho;
    *W = wo;
    return RN_OK;
}

/* ---- the three parts of a forward: input + stem + pool, a run of blocks, average pool + fc ---- */

/* The form the stem reads its image in (x4).  bf16: [B,H+6,W+6,4] with its own 3-pixel zero border,
 * padding 0.  fp32 exact-K: [B,H+6,W+6,3] with a physical border.  fp32 otherwise: [B,H,W,4] and the
 * layer's padding.  With from_nchw the fused stem + pool fetches its patches from the caller's NCHW fp32
 * image itself and no layout launch runs (a byte image always goes through x4).
 * The route is a function of (H, W, dtype, settings) alone, never of B: where the fused stem + pool launch
 * does not take the size (rn_stem_pool_applies: a conv output width off a multiple of 8 or above 128, its
 * LDS budget, an odd padded width in bf16), every launch of the model runs the stem and the max-pool as
 * separate launches, as with rn_model_set_stem_pool_fusion(m, 0); where only the NCHW-fetching form does
 * not (W % 4 != 0, W > 256), the padded-image form runs, which gives the same bits. */
typedef struct {
    uint64_t cpad, border; /* channels 3 or 4; zero border 0 or 3 */
    int exact, fused_pool, from_nchw;
} rn_stem_form;

static rn_stem_form stem_form(const rn_model *m, int in_u8, int mode)
{
    const int bf16 = m->dtype == RN_DTYPE_BF16;
    rn_stem_form f;
    f.exact = !bf16 && m->stem_exact;
    f.cpad = f.exact ? 3 : 4;
    f.border = bf16 || f.exact ? m->convs[0].pad : 0;
    f.fused_pool = mode == RN_FWD_FUSED && m->stem_pool && (bf16 || f.exact) &&
                   rn_stem_pool_applies(m->dtype, m->H + 2 * m->convs[0].pad, m->W + 2 * m->convs[0].pad, 0);
    f.from_nchw = f.fused_pool && m->stem_pool == 2 && !in_u8 &&
                  rn_stem_pool_applies(m->dtype, m->H + 2 * m->convs[0].pad, m->W + 2 * m->convs[0].pad, 1);
    return f;
}

/* The first launch: the caller's image -> the normalised (byte route) NHWC image in x4, the same bits
 * from 8-bit RGB [B,H,W,3] as from the host-normalised fp32 NCHW image. */
static const float kImageMean[3] = {0.485f, 0.456f, 0.406f}, kImageStd[3] = {0.229f, 0.224f, 0.225f};

static int op_input(rn_model *m, const void *input, int in_u8, uint64_t B, const rn_stem_form *f)
{
    const double out = (double)elem_size(m) * (double)((m->H + 2 * f->border) * (m->W + 2 * f->border)) * (double)f->cpad;
    const double in_numel = (double)(3 * m->H * m->W);
    TRY(prof_begin(m, in_u8 ? (f->cpad == 3 ? "image_u8_to_nhwc3" : "image_u8_to_nhwc4")
                            : (f->cpad == 3 ? "nchw_to_nhwc3" : "nchw_to_nhwc4"),
                   "input", 0.0, (double)B * ((in_u8 ? 1.0 : 4.0) * in_numel + out)));
    if (in_u8)
        TRY(rn_image_u8_to_nhwc_pad_dt(m->run.ctx, m->dtype, (const uint8_t *)input, m->run.x4, B, m->H, m->W,
                                       f->cpad, f->border, kImageMean, kImageStd));
    else
        TRY(rn_nchw_to_nhwc_pad_dt(m->run.ctx, m->dtype, (const float *)input, m->run.x4, B, 3, m->H, m->W,
                                   f->cpad, f->border));
    return prof_end(m);
}

/* conv1 + bn1 + ReLU + max-pool (main.cu:179-192) as one launch: x4 (physically padded image)
 * -> p0 (pooled, where the separate max-pool writes too).  Algorithmic work: the stem's FLOPs
 * (no halo), the image read once, the pooled tensor written once. */
static int op_stem_pool(rn_model *m, const rn_conv *stem, const float *input_nchw, uint64_t B,
                        const rn_stem_form *f)
{
    const double es = (double)elem_size(m);
    const uint64_t Hp = m->H + 2 * f->border, Wp = m->W + 2 * f->border;
    TRY(prof_begin(m, "conv2d+epilogue+maxpool", "conv1+maxpool",
                   2.0 * (double)(B * m->stem_h * m->stem_w) * (double)stem->cout *
                       (double)(stem->cin * stem->k * stem->k),
                   (input_nchw ? 4.0 * (double)(B * m->H * m->W * stem->cin)
                               : es * (double)(B * Hp * Wp) * (double)f->cpad) +
                       es * ((double)(stem->cout * stem->cin * stem->k * stem->k) +
                             (double)(B * m->pool_h * m->pool_w * stem->cout))));
    if (input_nchw) /* stem_pool == 2: the patch fetch reads the caller's NCHW fp32 image itself */
        TRY(rn_stem_pool_nchw_forward_dt(m->run.ctx, m->dtype, input_nchw, m->run.p0, m->stem_pool_packed,
                                         stem->scale, stem->shift, 1, B, stem->cin, m->H, m->W));
    else
        TRY(rn_stem_pool_forward_dt(m->run.ctx, m->dtype, m->run.x4, m->run.p0, m->stem_pool_packed, stem->scale,
                                    stem->shift, 1, B, Hp, Wp));
    return prof_end(m);
}

/* input + stem + max-pool: the caller's images -> p0 [B,pool_h,pool_w,64] */
static int run_front(rn_model *m, const void *input, int in_u8, uint64_t B, int mode)
{
    const rn_conv *stem = &m->convs[0];
    const rn_stem_form f = stem_form(m, in_u8, mode);
    const uint64_t Hp = m->H + 2 * f.border, Wp = m->W + 2 * f.border;
    const uint64_t so = m->stem_h * m->stem_w, po = m->pool_h * m->pool_w;
    rn_epilogue ep;
    if (!f.from_nchw) TRY(op_input(m, input, in_u8, B, &f));
    if (f.fused_pool) return op_stem_pool(m, stem, f.from_nchw ? (const float *)input : NULL, B, &f);
    ep.scale = stem->scale; ep.shift = stem->shift; ep.residual = NULL; ep.relu = 1;
    TRY(op_conv_at(m, stem, m->run.x4, m->run.p1, B, Hp, Wp, mode == RN_FWD_FUSED ? &ep : NULL,
                   f.border ? 0 : stem->pad, f.exact));
    if (mode != RN_FWD_FUSED) {
        TRY(op_bn(m, stem, m->run.p1, B, so));
        TRY(op_relu(m, "conv1", m->run.p1, B * so * stem->cout));
    }
    /* maxpool 3x3 s2 p1 (main.cu:114,192) */
    TRY(prof_begin(m, "maxpool2d", "maxpool", 0.0,
                   (double)elem_size(m) * (double)(B * stem->cout * (so + po))));
    TRY(rn_maxpool2d_nhwc_forward_dt(m->run.ctx, m->dtype, m->run.p1, m->run.p0, 3, 2, 1, m->pool_h, m->pool_w, B,
                                     stem->cout, m->stem_h, m->stem_w));
    return prof_end(m);
}

/* block i reads ping-pong arena i & 1 and writes the other */
static float *block_input(const rn_model *m, int i) { return (i & 1) ? m->run.p1 : m->run.p0; }

/* rn_model_forward_maps: stage li + 1's output x [B,H,W,C] of this launch -> the caller's NCHW fp32 map, from the
 * caller's image run.img0 on.  Queued right behind the stage's last block on that block's stream: two blocks
 * later the same stream overwrites the arena x lives in. */
static int op_stage_map(rn_model *m, int li, const float *x, uint64_t B, uint64_t H, uint64_t W)
{
    const uint64_t C = m->basic ? kBasicWidths[li] : kWidths[li][2];
    char layer[RN_MAX_KEY];
    snprintf(layer, sizeof(layer), "layer%d", li + 1);
    TRY(prof_begin(m, "stage_map", layer, 0.0, (double)(B * C * H * W) * (double)(elem_size(m) + 4)));
    TRY(rn_nhwc_to_nchw_dt(m->run.ctx, m->dtype, x, m->maps->layer[li] + m->run.img0 * C * H * W, B, C, H, W));
    return prof_end(m);
}

/* rn_model_forward_segment: the head on layer4's output x [B,h,w,C] of this launch, into the caller's buffers from
 * image run.img0 on.  Queued behind the last block on that block's stream, like op_stage_map and for its reason.
 * The launch's images use the slice of the head's scratch that starts at their index in the sub-batch: the parts
 * of a launch batch run side by side on their streams, and forward_chunk joins those streams before the next
 * sub-batch reuses the scratch, as it does for the arenas. */
static int op_segment(rn_model *m, const float *x, uint64_t B, uint64_t h, uint64_t w)
{
    const uint64_t HW = m->H * m->W;
    uint64_t d[4]; /* in, mid, classes, padded classes */
    float *scores;
    uint8_t *labels;
    int step, steps;
    rn_seg_head_dims(m->seg_head, d);
    scores = m->seg->scores ? m->seg->scores + m->run.img0 * d[2] * HW : NULL;
    labels = m->seg->labels ? m->seg->labels + m->run.img0 * HW : NULL;
    /* the head says what it launches: three steps (FCN) or rates + 8 (DeepLab), with their names, FLOPs and bytes */
    steps = rn_seg_head_plan(m->seg_head, B, h, w, m->H, m->W, scores != NULL, labels != NULL, -1, NULL, NULL, NULL);
    for (step = 0; step < steps; ++step) {
        const char *op = NULL;
        double flops = 0.0, bytes = 0.0;
        rn_seg_head_plan(m->seg_head, B, h, w, m->H, m->W, scores != NULL, labels != NULL, step, &op, &flops, &bytes);
        TRY(prof_begin(m, op, "segmentation", flops, bytes));
        TRY(rn_seg_head_step(m->seg_head, m->run.ctx, step, x, m->run.sub0, B, h, w, m->H, m->W, scores, labels));
        TRY(prof_end(m));
    }
    return RN_OK;
}

/* rn_model_forward_fpn: the lateral 1x1 of the level that reads stage li + 1, on the stage's output x in place.
 * Queued right behind the stage's last block on that block's stream, like op_stage_map and for its reason.  The
 * images of this launch use the slice of the neck's scratch that starts at their index in the sub-batch, for
 * op_segment's reason. */
static int op_fpn_lateral(rn_model *m, int li, const float *x, uint64_t B)
{
    const rn_neck_call *c = m->neck;
    int j;
    for (j = 0; j < c->n; ++j) {
        double flops = 0.0, bytes = 0.0;
        if (m->fpn_stage[j] != li + 1) continue;
        rn_fpn_cost(c->fpn, RN_FPN_INNER, j, B, c->h, c->w, &flops, &bytes);
        TRY(prof_begin(m, rn_fpn_op_name(c->fpn, RN_FPN_INNER, j), "fpn", flops, bytes));
        TRY(rn_fpn_step(c->fpn, m->run.ctx, RN_FPN_INNER, j, x, m->run.sub0, B, c->h, c->w, NULL));
        TRY(prof_end(m));
    }
    return RN_OK;
}

/* rn_model_forward_fpn: what follows the laterals, behind the last block of all (where op_segment sits): the steps
 * of rn_neck_plan for this part's images, each under its own profile record */
static int op_fpn_rest(rn_model *m, uint64_t B)
{
    const int steps = rn_neck_plan(m->neck, B, -1, NULL, NULL, NULL, NULL);
    int step;
    for (step = 0; step < steps; ++step) {
        const char *op = NULL, *layer = NULL;
        double flops = 0.0, bytes = 0.0;
        rn_neck_plan(m->neck, B, step, &op, &layer, &flops, &bytes);
        TRY(prof_begin(m, op, layer, flops, bytes));
        TRY(rn_neck_step(m->neck, m->run.ctx, step, m->run.sub0, m->run.img0, B));
        TRY(prof_end(m));
    }
    return RN_OK;
}

/* blocks [first, last) on an *H x *W map, which become those of block last's input; behind the last block of a
 * stage the export of its map or the neck's lateral on it, when the running call wants either; behind the last block
 * of all the segmentation head or the rest of the neck */
static int run_blocks(rn_model *m, int first, int last, uint64_t B, uint64_t *H, uint64_t *W, int mode)
{
    int bi, li = 0, end = m->depths[0]; /* block `end` is the first of stage li + 1 */
    for (bi = first; bi < last; ++bi) {
        TRY(block_forward(m, &m->blocks[bi], block_input(m, bi), block_input(m, bi + 1), B, H, W, mode));
        while (bi >= end) end += m->depths[++li];
        if (m->maps && bi + 1 == end && m->maps->layer[li]) TRY(op_stage_map(m, li, block_input(m, bi + 1), B, *H, *W));
        if (m->seg_head && bi + 1 == m->n_blocks) TRY(op_segment(m, block_input(m, bi + 1), B, *H, *W));
        if (m->neck && bi + 1 == end) TRY(op_fpn_lateral(m, li, block_input(m, bi + 1), B));
        if (m->neck && bi + 1 == m->n_blocks) TRY(op_fpn_rest(m, B));
    }
    return RN_OK;
}

/* global average over the H x W map (main.cu:120,213: 7 x 7, where this is that launch) then fc (main.cu:122,224) */
static int run_head(rn_model *m, const float *x, uint64_t B, uint64_t H, uint64_t W, float *logits)
{
    const double es = (double)elem_size(m);
    TRY(prof_begin(m, "avgpool2d", "avgpool", 0.0, es * (double)(B * m->feat * (H * W + 1))));
    TRY(rn_global_avgpool_nhwc_forward_dt(m->run.ctx, m->dtype, x, m->run.pooled, B, m->feat, H, W));
    TRY(prof_end(m));
    TRY(prof_begin(m, "linear", "fc", 2.0 * (double)B * (double)m->feat * (double)m->classes,
                   es * ((double)(B * m->feat) + (double)m->feat * (double)m->classes) +
                       4.0 * ((double)m->classes + (double)B * (double)m->classes)));
    if (m->dtype == RN_DTYPE_BF16) {
        rn_epilogue ep;
        ep.scale = NULL; ep.shift = m->params[m->fc_b].dev; ep.residual = NULL; ep.relu = 0;
        TRY(rn_conv2d_nhwc_forward_dt(m->run.ctx, m->dtype, RN_DTYPE_F32, m->run.pooled, logits, m->fc_packed, 1, 1, 0,
                                      1, 1, B, m->feat, m->classes, 1, 1, &ep));
    } else if (m->classes % 4 != 0) {
        /* the rows of a later part or sub-batch start off a 16-byte boundary, where rn_linear_forward takes the
         * direct kernel: every launch of this layer takes it, so that an image's logits do not depend on the
         * part it runs in */
        TRY(rn_linear_direct_forward(m->run.ctx, m->run.pooled, logits, m->params[m->fc_w].dev,
                                     m->params[m->fc_b].dev, B, m->feat, m->classes));
    } else {
        TRY(rn_linear_forward(m->run.ctx, m->run.pooled, logits, m->params[m->fc_w].dev, m->params[m->fc_b].dev, B,
                              m->feat, m->classes));
    }
    return prof_end(m);
}

/* What the ops queued from here on run on: context `ctx`, mode, and the arenas from image img_off +
 * slice_off on.  slice_off: images into the part of a slice of a depth-first front.  The back phase reads
 * the first stage's output of all slices as one batch, so in the ping-pong arenas a slice starts slice_off
 * first-stage outputs into its part (in a basic-block network 1/4 of an arena image; the slice's larger
 * stem tensor then reaches into the room of the slices after it, which run later on the same stream). */
static void run_begin(rn_model *m, rn_ctx *ctx, uint64_t img_off, uint64_t slice_off, int mode)
{
    const uint64_t es = elem_size(m);
    const uint64_t p_off = img_off * m->p_img + slice_off * m->s1_img;
    rn_run *r = &m->run;
    img_off += slice_off;
    r->ctx = ctx;
    r->mode = mode;
    r->t1_ready = 0;
    r->img0 = m->maps_done + img_off;
    r->sub0 = img_off;
    r->x4 = (float *)((char *)m->x4 + img_off * m->x4_img * es);
    r->p0 = (float *)((char *)m->p0 + p_off * es);
    r->p1 = (float *)((char *)m->p1 + p_off * es);
    r->dsb = (float *)((char *)m->dsb + img_off * m->ds_img * es);
    r->t1 = (float *)((char *)m->t1 + img_off * m->t1_img * es);
    r->t2 = m->t2 ? (float *)((char *)m->t2 + img_off * m->t2_img * es) : NULL; /* none in a basic block */
    r->pooled = (float *)((char *)m->pooled + img_off * m->feat * es);
}

/* a whole forward, or the halves of a depth-first one: the front ends after the first stage, where the
 * back (the front ran already, in slices) starts */
enum { RN_PHASE_ALL = 0, RN_PHASE_FRONT = 1, RN_PHASE_BACK = 2 };

static int forward_phase(rn_model *m, const void *input, int in_u8, uint64_t B, float *logits, int mode,
                         int phase)
{
    const int first = phase == RN_PHASE_BACK ? m->depths[0] : 0;
    const int last = phase == RN_PHASE_FRONT ? m->depths[0] : m->n_blocks;
    uint64_t H = m->pool_h, W = m->pool_w; /* the first stage keeps them (stride 1): the back starts there too */
    if (phase != RN_PHASE_BACK) TRY(run_front(m, input, in_u8, B, mode));
    TRY(run_blocks(m, first, last, B, &H, &W, mode));
    if (phase != RN_PHASE_FRONT) TRY(run_head(m, block_input(m, last), B, H, W, logits));
    return RN_OK;
}

/* B images whose activations live at image offset img_off (+ slice_off) of the arenas, queued on `run` */
static int forward_sub(rn_model *m, rn_ctx *run, uint64_t img_off, uint64_t slice_off, const void *input,
                       int in_u8, uint64_t B, float *logits, int mode, int phase)
{
    const int saved_layout = rn_ctx_get_layout(run);
    int st;
    run_begin(m, run, img_off, slice_off, mode);
    rn_ctx_set_layout(run, RN_LAYOUT_NHWC);
    st = forward_phase(m, input, in_u8, B, logits, mode, phase);
    rn_ctx_set_layout(run, saved_layout);
    return st;
}

/* smallest batch part worth a stream of its own.  bf16 launches are short (fill and drain are a
 * third of their life): parts of 64 still gain 6-8 %.  fp32 launches are matrix-bound rounds of
 * tiles: parts of 128 gain 1 %, parts of 96 LOSE 3 % (B = 192), parts of 64 nothing
 * (tools/streams_ab.sh) -- so the library's own default of two streams starts at parts of 128 there;
 * a count the caller set (rn_model_set_streams) is taken down to parts of 64 */
#define RN_STREAM_MIN_PART(m) ((m)->dtype == RN_DTYPE_F32 && !(m)->streams_set ? 128u : 64u)

/* parts (streams) a launch batch of B images runs as */
static int parts_of(const rn_model *m, uint64_t B)
{
    int parts = m->streams;
    if (B > m->max_sub) B = m->max_sub; /* images per launch batch: see rn_model_forward */
    while (parts > 1 && B / (uint64_t)parts < RN_STREAM_MIN_PART(m)) parts /= 2;
    return parts;
}
#define RN_FRONT_MIN_SLICE 16

/* image `lo` of the caller's input: fp32 NCHW, or 8-bit RGB on the byte route */
static const void *input_at(const rn_model *m, const void *input, int in_u8, uint64_t lo)
{
    return (const char *)input + lo * 3 * m->H * m->W * (in_u8 ? 1 : sizeof(float));
}

/* B images at image offset img_off on `run`: whole, or depth-first through the front */
static int forward_part(rn_model *m, rn_ctx *run, uint64_t img_off, const void *input, int in_u8,
                        uint64_t B, float *logits, int mode)
{
    int fp = m->front_parts, j;
    uint64_t lo = 0;
    while (fp > 1 && B / (uint64_t)fp < RN_FRONT_MIN_SLICE) fp /= 2;
    if (fp < 2) return forward_sub(m, run, img_off, 0, input, in_u8, B, logits, mode, RN_PHASE_ALL);
    for (j = 0; j < fp; ++j) {
        const uint64_t hi = B * (uint64_t)(j + 1) / (uint64_t)fp;
        TRY(forward_sub(m, run, img_off, lo, input_at(m, input, in_u8, lo), in_u8, hi - lo, logits, mode,
                        RN_PHASE_FRONT));
        lo = hi;
    }
    return forward_sub(m, run, img_off, 0, input, in_u8, B, logits, mode, RN_PHASE_BACK);
}

/* One sub-batch: every tensor of it stays below the kernels' 2^29-element range.  Large enough,
 * it runs as `streams` contiguous parts on as many streams (see rn_model.streams).  prof_keep: the
 * profile records queued before it (the resize launch) stay. */
static int forward_chunk(rn_model *m, const void *input, int in_u8, uint64_t B, float *logits, int mode,
                         int prof_keep)
{
    uint64_t lo = 0;
    int parts = parts_of(m, B), i;
    TRY(ensure_acts(m, B));
    if (!prof_keep) m->n_prof = 0;
    if (parts < 2 || m->profiling || m->single_stream_only || m->recording)
        return forward_part(m, m->ctx, 0, input, in_u8, B, logits, mode);
    if (!m->ev_fork) TRY(rn_event_create(m->ctx, &m->ev_fork));
    for (i = 0; i < parts - 1; ++i) {
        if (m->ctxn[i]) continue;
        TRY(rn_ctx_create(&m->ctxn[i], rn_ctx_device(m->ctx), NULL));
        TRY(rn_event_create(m->ctxn[i], &m->ev_join[i]));
    }
    /* fork: whatever the caller queued before this forward (the input upload) is done before
     * the other streams start; join: the first stream carries on after every part */
    TRY(rn_event_record(m->ctx, m->ev_fork));
    for (i = 0; i < parts; ++i) {
        const uint64_t hi = B * (uint64_t)(i + 1) / (uint64_t)parts;
        rn_ctx *run = i == 0 ? m->ctx : m->ctxn[i - 1];
        if (i > 0) {
            TRY(rn_ctx_set_tap_skip(run, rn_ctx_tap_skip_mode(m->ctx))); /* the caller's choice holds on every stream */
            TRY(rn_ctx_wait_event(run, m->ev_fork));
        }
        TRY(forward_part(m, run, lo, input_at(m, input, in_u8, lo), in_u8, hi - lo, logits + lo * m->classes,
                         mode));
        if (i > 0) TRY(rn_event_record(run, m->ev_join[i - 1]));
        lo = hi;
    }
    for (i = 0; i < parts - 1; ++i) TRY(rn_ctx_wait_event(m->ctx, m->ev_join[i]));
    return RN_OK;
}

/* What rn_model_forward_outputs adds behind the launches of a sub-batch of nb images (the caller's image
 * `done` on), on the model's own stream, which every part has joined: the features out of `pooled`, then at
 * most one launch of the head kernel on the sub-batch's logits. */
static int head_outputs(rn_model *m, const rn_model_outputs *o, uint64_t done, uint64_t nb, const float *logits)
{
    const uint64_t C = m->classes;
    m->run.ctx = m->ctx; /* the profile brackets of these launches */
    if (o->features) {
        float *dst = o->features + done * m->feat;
        TRY(prof_begin(m, "features", "head", 0.0, (double)(nb * m->feat) * (double)(elem_size(m) + 4)));
        if (m->dtype == RN_DTYPE_BF16)
            TRY(rn_widen_bf16_forward(m->ctx, m->pooled, dst, nb * m->feat));
        else
            TRY(rn_memcpy_d2d(m->ctx, dst, m->pooled, nb * m->feat * sizeof(float)));
        TRY(prof_end(m));
    }
    if (o->k > 0) {
        const double bytes = 4.0 * (double)(nb * C) * (o->probs ? 2.0 : 1.0) + 12.0 * (double)(nb * o->k);
        TRY(prof_begin(m, "softmax_topk", "head", 0.0, bytes));
        TRY(rn_softmax_topk_forward(m->ctx, logits, o->probs ? o->probs + done * C : NULL, o->topk_prob + done * o->k,
                                    o->topk_idx + done * o->k, nb, C, o->k));
        TRY(prof_end(m));
    } else if (o->probs) {
        TRY(prof_begin(m, "softmax", "head", 0.0, 8.0 * (double)(nb * C)));
        TRY(rn_softmax_forward(m->ctx, logits, o->probs + done * C, nb, C));
        TRY(prof_end(m));
    }
    return RN_OK;
}

/* The reference has no batch limit other than memory (main.cu:168-226).  Here the contraction
 * kernels address every tensor with 32-bit byte offsets (2^29 fp32 elements; at 224 x 224 the stem
 * output of 669 images is the first to pass it), so a larger batch runs as sub-batches of at most
 * m->max_sub images (set_geometry: 512 at 224 x 224, fewer for larger images) through the same arenas.
 * Every image's logits are independent of what else is in its launch (batch invariance, bit for bit), so
 * the split changes nothing.
 * in_u8: the input is 8-bit RGB [B,H,W,3], not fp32 NCHW; prof_keep: see forward_chunk (the
 * first sub-batch only).  outs (rn_model_forward_outputs, NULL otherwise): what to write besides the
 * logits; with logits == NULL those of a sub-batch go to a buffer the model owns. */
static int forward_outputs(rn_model *m, const void *input, int in_u8, uint64_t B, float *logits,
                           const rn_model_outputs *outs, int mode, int prof_keep)
{
    uint64_t done = 0;
    if (!m || !input || (!logits && !outs) || B == 0) return RN_ERR_INVALID;
    if (mode != RN_FWD_REFERENCE_OPS && mode != RN_FWD_FUSED) return RN_ERR_INVALID;
    if (!m->finalized) return RN_ERR_INVALID;
    /* bf16 storage exists only with the fused epilogues (no standalone bf16 bn/relu/add) */
    if (m->dtype != RN_DTYPE_F32 && mode != RN_FWD_FUSED) return RN_ERR_UNSUPPORTED;
    if (outs) {
        if (!logits && !outs->features && !outs->probs && outs->k == 0 && !m->maps && !m->seg_head && !m->neck) return RN_ERR_INVALID;
        if (outs->k > 0 && (!outs->topk_prob || !outs->topk_idx || outs->k > 64 || outs->k > m->classes))
            return RN_ERR_INVALID;
    }
    if (!logits) {
        const uint64_t need = B < m->max_sub ? B : m->max_sub;
        if (need > m->own_logits_cap) { /* grows like the arenas: never under a capture or a live graph */
            if (rn_ctx_is_capturing(m->ctx)) return RN_ERR_UNSUPPORTED;
            if (m->own_logits_cap > 0 && rn_ctx_graphs_live(m->ctx) > 0) return RN_ERR_INVALID;
            if (m->own_logits) TRY(rn_free(m->ctx, m->own_logits));
            m->own_logits = NULL;
            m->own_logits_cap = 0;
            TRY(rn_malloc(m->ctx, (void **)&m->own_logits, need * m->classes * sizeof(float)));
            m->own_logits_cap = need;
        }
    }
    while (done < B) {
        const uint64_t nb = B - done < m->max_sub ? B - done : m->max_sub;
        float *sub = logits ? logits + done * m->classes : m->own_logits;
        m->maps_done = done;
        TRY(forward_chunk(m, input_at(m, input, in_u8, done), in_u8, nb, sub, mode, prof_keep && done == 0));
        if (outs) TRY(head_outputs(m, outs, done, nb, sub));
        done += nb;
    }
    return RN_OK;
}

static int forward_any(rn_model *m, const void *input, int in_u8, uint64_t B, float *logits, int mode,
                       int prof_keep)
{
    return forward_outputs(m, input, in_u8, B, logits, NULL, mode, prof_keep);
}

int rn_model_forward(rn_model *m, const float *input_nchw, uint64_t B, float *logits, int mode)
{
    return forward_any(m, input_nchw, 0, B, logits, mode, 0);
}

int rn_model_forward_u8(rn_model *m, const uint8_t *input_nhwc, uint64_t B, float *logits, int mode)
{
    return forward_any(m, input_nhwc, 1, B, logits, mode, 0);
}

int rn_model_forward_outputs(rn_model *m, const float *input_nchw, uint64_t B, const rn_model_outputs *outs, int mode)
{
    if (!outs) return RN_ERR_INVALID;
    return forward_outputs(m, input_nchw, 0, B, outs->logits, outs, mode, 0);
}

int rn_model_forward_outputs_u8(rn_model *m, const uint8_t *input_nhwc, uint64_t B, const rn_model_outputs *outs,
                                int mode)
{
    if (!outs) return RN_ERR_INVALID;
    return forward_outputs(m, input_nhwc, 1, B, outs->logits, outs, mode, 0);
}

/* rn_model_forward_maps(_u8): the request is state of this call alone -- set once every refusal that belongs to the
 * maps has passed, cleared on every way out -- so that no other forward, tuning pass, capture or pipeline submit
 * ever exports (run_blocks asks m->maps). */
static int forward_maps(rn_model *m, const void *input, int in_u8, uint64_t B, const rn_model_outputs *outs,
                        const rn_model_maps *maps, int mode)
{
    rn_model_outputs none;
    int li, wanted = 0, st;
    if (!m) return RN_ERR_INVALID;
    if (!maps) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_maps: maps is NULL");
    for (li = 0; li < 4; ++li) {
        if (!maps->layer[li]) continue;
        wanted = 1;
        if ((uintptr_t)maps->layer[li] & 3) {
            char msg[96];
            snprintf(msg, sizeof(msg), "rn_model_forward_maps: the map of layer%d must be 4-byte aligned", li + 1);
            return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, msg);
        }
    }
    if (!wanted && !(outs && (outs->logits || outs->features || outs->probs || outs->k)))
        return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_maps: nothing to write");
    memset(&none, 0, sizeof(none));
    if (!outs) outs = &none;
    m->maps = wanted ? maps : NULL;
    st = forward_outputs(m, input, in_u8, B, outs->logits, outs, mode, 0);
    m->maps = NULL;
    m->maps_done = 0;
    return st;
}

int rn_model_forward_maps(rn_model *m, const float *input_nchw, uint64_t B, const rn_model_outputs *outs,
                          const rn_model_maps *maps, int mode)
{
    return forward_maps(m, input_nchw, 0, B, outs, maps, mode);
}

int rn_model_forward_maps_u8(rn_model *m, const uint8_t *input_nhwc, uint64_t B, const rn_model_outputs *outs,
                             const rn_model_maps *maps, int mode)
{
    return forward_maps(m, input_nhwc, 1, B, outs, maps, mode);
}

/* rn_model_forward_segment(_u8): like the maps, the request is state of this call alone -- set once every refusal
 * has passed, cleared on every way out (run_blocks asks m->seg_head). */
static int forward_segment(rn_model *m, rn_seg_head *hd, const void *input, int in_u8, uint64_t B,
                           const rn_model_outputs *outs, const rn_seg_outputs *seg, int mode)
{
    rn_model_outputs none;
    const char *why = NULL;
    uint64_t h = 0, w = 0;
    int st;
    if (!m) return RN_ERR_INVALID;
    if (!seg) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_segment: seg is NULL");
    if (!seg->labels && !seg->scores)
        return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_segment: seg names nothing (labels and scores are NULL)");
    if ((uintptr_t)seg->scores & 3)
        return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_segment: seg->scores must be 4-byte aligned");
    if (!m->finalized) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_segment: the model is not finalized");
    if (!rn_seg_head_matches(hd, m->feat, m->dtype, &why)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "rn_model_forward_segment: %s", why);
        return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, msg);
    }
    if (!input || B == 0 || (mode != RN_FWD_REFERENCE_OPS && mode != RN_FWD_FUSED)) return RN_ERR_INVALID;
    if (m->dtype != RN_DTYPE_F32 && mode != RN_FWD_FUSED) return RN_ERR_UNSUPPORTED;
    TRY(rn_model_stage_shape(m, 4, NULL, &h, &w));
    TRY(rn_seg_head_reserve(hd, B < m->max_sub ? B : m->max_sub, h * w));
    memset(&none, 0, sizeof(none));
    if (!outs) outs = &none;
    m->seg_head = hd;
    m->seg = seg;
    st = forward_outputs(m, input, in_u8, B, outs->logits, outs, mode, 0);
    m->seg_head = NULL;
    m->seg = NULL;
    m->maps_done = 0;
    return st;
}

int rn_model_forward_segment(rn_model *m, rn_seg_head *hd, const float *input_nchw, uint64_t B,
                             const rn_model_outputs *outs, const rn_seg_outputs *seg, int mode)
{
    return forward_segment(m, hd, input_nchw, 0, B, outs, seg, mode);
}

int rn_model_forward_segment_u8(rn_model *m, rn_seg_head *hd, const uint8_t *input_nhwc, uint64_t B,
                                const rn_model_outputs *outs, const rn_seg_outputs *seg, int mode)
{
    return forward_segment(m, hd, input_nhwc, 1, B, outs, seg, mode);
}

/* rn_model_forward_fpn and the entry points that run more behind its neck (fn names the one that was called; c holds
 * what it was given).  The model's own refusals -- the stages and their channel counts -- then the neck call's check
 * against the head outputs, then the reserve.  Like the maps, the call is state of this forward alone: set once every
 * refusal has passed, cleared on every way out (run_blocks asks m->neck). */
static int forward_fpn(rn_model *m, const char *fn, rn_neck_call *c, const void *input, int in_u8, uint64_t B,
                       const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fo, int mode)
{
    static const rn_fpn_outputs no_levels = {{NULL, NULL, NULL, NULL, NULL}};
    rn_model_outputs none;
    const char *why = NULL;
    char msg[200];
    uint64_t cin[4];
    int n = 0, j, st;
    if (!m) return RN_ERR_INVALID;
    if (!m->finalized) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_fpn: the model is not finalized");
    if (!rn_fpn_matches(c->fpn, m->ctx, m->dtype, &why)) {
        snprintf(msg, sizeof(msg), "rn_model_forward_fpn: %s", why);
        return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, msg);
    }
    if (!stages) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_fpn: stages is NULL");
    if (!fo && (c->roi || c->rpn)) fo = &no_levels;
    if (!fo) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_fpn: fpn_out is NULL");
    rn_fpn_dims(c->fpn, &n, NULL, NULL, cin);
    for (j = 0; j < n; ++j)
        if (stages[j] < 1 || stages[j] > 4 || (j > 0 && stages[j] <= stages[j - 1]))
            return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_fpn: stages must be ascending, each 1..4");
    for (j = 0; j < n; ++j) {
        uint64_t C = 0;
        TRY(rn_model_stage_shape(m, stages[j], &C, &c->h[j], &c->w[j]));
        if (C != cin[j]) {
            snprintf(msg, sizeof(msg), "rn_model_forward_fpn: in_channels of level %d is %llu, layer%d has %llu channels", j,
                     (unsigned long long)cin[j], stages[j], (unsigned long long)C);
            return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, msg);
        }
    }
    memset(&none, 0, sizeof(none));
    if (!outs) outs = &none;
    c->out = fo->level, c->image_h = m->H, c->image_w = m->W, c->images = B;
    {
        const rn_operand heads[5] = {{outs->logits, B * m->classes * sizeof(float), "logits", 1, 0},
                                     {outs->features, B * m->feat * sizeof(float), "features", 1, 0},
                                     {outs->probs, B * m->classes * sizeof(float), "probs", 1, 0},
                                     {outs->topk_prob, B * outs->k * sizeof(float), "topk_prob", 1, 0},
                                     {outs->topk_idx, B * outs->k * sizeof(uint64_t), "topk_idx", 1, 0}};
        TRY(rn_neck_check(c, m->ctx, fn, heads, 5));
    }
    if (!input || B == 0 || (mode != RN_FWD_REFERENCE_OPS && mode != RN_FWD_FUSED)) return RN_ERR_INVALID;
    if (m->dtype != RN_DTYPE_F32 && mode != RN_FWD_FUSED)
        return rn_ctx_set_error(m->ctx, RN_ERR_UNSUPPORTED, "rn_model_forward_fpn: a bf16 model runs RN_FWD_FUSED only");
    TRY(rn_neck_reserve(c, B < m->max_sub ? B : m->max_sub));
    for (j = 0; j < n; ++j) m->fpn_stage[j] = stages[j];
    m->neck = c;
    st = forward_outputs(m, input, in_u8, B, outs->logits, outs, mode, 0);
    m->neck = NULL;
    m->maps_done = 0;
    return st;
}

/* what an entry point of the forward_fpn family was given, the rest zero */
static rn_neck_call neck_call(rn_fpn *fpn, const rn_roi_pool *rois, rn_rpn *rpn, const rn_rpn_request *req, rn_box_head *bh,
                              const rn_detect_request *det_req)
{
    rn_neck_call c;
    memset(&c, 0, sizeof(c));
    c.fpn = fpn, c.roi = rois, c.rpn = rpn, c.rpn_req = req, c.box_head = bh, c.det_req = det_req;
    return c;
}

int rn_model_forward_fpn(rn_model *m, rn_fpn *fpn, const float *input_nchw, uint64_t B, const rn_model_outputs *outs,
                         const int *stages, const rn_fpn_outputs *fpn_out, int mode)
{
    rn_neck_call c = neck_call(fpn, NULL, NULL, NULL, NULL, NULL);
    return forward_fpn(m, __func__, &c, input_nchw, 0, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_fpn_u8(rn_model *m, rn_fpn *fpn, const uint8_t *input_nhwc, uint64_t B, const rn_model_outputs *outs,
                            const int *stages, const rn_fpn_outputs *fpn_out, int mode)
{
    rn_neck_call c = neck_call(fpn, NULL, NULL, NULL, NULL, NULL);
    return forward_fpn(m, "rn_model_forward_fpn", &c, input_nhwc, 1, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_rois(rn_model *m, rn_fpn *fpn, const float *input_nchw, uint64_t B, const rn_model_outputs *outs,
                          const int *stages, const rn_fpn_outputs *fpn_out, const rn_roi_pool *rois, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, NULL, NULL, NULL, NULL);
    if (m && !rois) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_rois: rois is NULL");
    return forward_fpn(m, __func__, &c, input_nchw, 0, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_rois_u8(rn_model *m, rn_fpn *fpn, const uint8_t *input_nhwc, uint64_t B, const rn_model_outputs *outs,
                             const int *stages, const rn_fpn_outputs *fpn_out, const rn_roi_pool *rois, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, NULL, NULL, NULL, NULL);
    if (m && !rois) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_rois: rois is NULL");
    return forward_fpn(m, "rn_model_forward_rois", &c, input_nhwc, 1, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_proposals(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, const float *input_nchw, uint64_t B,
                               const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                               const rn_rpn_request *req, const rn_roi_pool *rois, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, rpn, req, NULL, NULL);
    if (m && (!rpn || !req)) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_proposals: rpn or req is NULL");
    return forward_fpn(m, __func__, &c, input_nchw, 0, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_proposals_u8(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, const uint8_t *input_nhwc, uint64_t B,
                                  const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                                  const rn_rpn_request *req, const rn_roi_pool *rois, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, rpn, req, NULL, NULL);
    if (m && (!rpn || !req)) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_proposals: rpn or req is NULL");
    return forward_fpn(m, "rn_model_forward_proposals", &c, input_nhwc, 1, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_detections(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, const float *input_nchw, uint64_t B,
                                const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                                const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, rpn, req, bh, det_req);
    if (m && (!rpn || !req)) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_detections: rpn or req is NULL");
    if (m && (!bh || !det_req))
        return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_detections: the box head or its request is NULL");
    return forward_fpn(m, __func__, &c, input_nchw, 0, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_detections_u8(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, const uint8_t *input_nhwc, uint64_t B,
                                   const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                                   const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, rpn, req, bh, det_req);
    if (m && (!rpn || !req)) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_detections: rpn or req is NULL");
    if (m && (!bh || !det_req))
        return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_detections: the box head or its request is NULL");
    return forward_fpn(m, "rn_model_forward_detections", &c, input_nhwc, 1, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_masks(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh, const float *input_nchw,
                           uint64_t B, const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                           const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req,
                           const rn_mask_request *mask_req, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, rpn, req, bh, det_req);
    rn_mask_head_slot(mh, mask_req, &c.head[RN_NECK_MASK_SLOT]);
    if (m && (!rpn || !req)) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_masks: rpn or req is NULL");
    if (m && !mh) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_masks: the mask head is NULL");
    return forward_fpn(m, __func__, &c, input_nchw, 0, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_masks_u8(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh, const uint8_t *input_nhwc,
                              uint64_t B, const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                              const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req,
                              const rn_mask_request *mask_req, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, rpn, req, bh, det_req);
    rn_mask_head_slot(mh, mask_req, &c.head[RN_NECK_MASK_SLOT]);
    if (m && (!rpn || !req)) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_masks: rpn or req is NULL");
    if (m && !mh) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_masks: the mask head is NULL");
    return forward_fpn(m, "rn_model_forward_masks", &c, input_nhwc, 1, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_keypoints(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh, rn_keypoint_head *kh,
                               const float *input_nchw, uint64_t B, const rn_model_outputs *outs, const int *stages,
                               const rn_fpn_outputs *fpn_out, const rn_rpn_request *req, const rn_roi_pool *rois,
                               const rn_detect_request *det_req, const rn_mask_request *mask_req, const rn_keypoint_request *kp_req,
                               int mode)
{
    rn_neck_call c = neck_call(fpn, rois, rpn, req, bh, det_req);
    rn_mask_head_slot(mh, mask_req, &c.head[RN_NECK_MASK_SLOT]), rn_keypoint_head_slot(kh, kp_req, &c.head[RN_NECK_KEYPOINT_SLOT]);
    if (m && (!rpn || !req)) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_keypoints: rpn or req is NULL");
    if (m && !kh) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_keypoints: the keypoint head is NULL");
    return forward_fpn(m, __func__, &c, input_nchw, 0, B, outs, stages, fpn_out, mode);
}

int rn_model_forward_keypoints_u8(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh, rn_keypoint_head *kh,
                                  const uint8_t *input_nhwc, uint64_t B, const rn_model_outputs *outs, const int *stages,
                                  const rn_fpn_outputs *fpn_out, const rn_rpn_request *req, const rn_roi_pool *rois,
                                  const rn_detect_request *det_req, const rn_mask_request *mask_req,
                                  const rn_keypoint_request *kp_req, int mode)
{
    rn_neck_call c = neck_call(fpn, rois, rpn, req, bh, det_req);
    rn_mask_head_slot(mh, mask_req, &c.head[RN_NECK_MASK_SLOT]), rn_keypoint_head_slot(kh, kp_req, &c.head[RN_NECK_KEYPOINT_SLOT]);
    if (m && (!rpn || !req)) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_keypoints: rpn or req is NULL");
    if (m && !kh) return rn_ctx_set_error(m->ctx, RN_ERR_INVALID, "rn_model_forward_keypoints: the keypoint head is NULL");
    return forward_fpn(m, "rn_model_forward_keypoints", &c, input_nhwc, 1, B, outs, stages, fpn_out, mode);
}

/* The decoded-image route resizes to 256 and crops 224 x 224: a model of another size refuses it. */
static int default_size(const rn_model *m) { return m->H == RN_DEFAULT_SIDE && m->W == RN_DEFAULT_SIDE; }

static int images_need_default(rn_model *m)
{
    return rn_ctx_set_error(m->ctx, RN_ERR_UNSUPPORTED,
                            "decoded images are resized to 256 and cropped to 224 x 224: the model's input size is "
                            "another (rn_model_set_input_size); crop them yourself and use rn_model_forward_u8");
}

/* Decoded images whose tables are on the device already (the host pipeline stages them with the batch):
 * one resize launch for the whole batch on the model's stream, then the byte route on the crops.
 * src_bytes: what the launch reads, for the profile record. */
int rn_model_forward_images_table(rn_model *m, const uint8_t *packed_dev, const void *table_dev, uint64_t B,
                                  double src_bytes, float *logits, int mode)
{
    if (!m || !packed_dev || !table_dev || !logits || B == 0) return RN_ERR_INVALID;
    if (mode != RN_FWD_REFERENCE_OPS && mode != RN_FWD_FUSED) return RN_ERR_INVALID;
    if (!m->finalized) return RN_ERR_INVALID;
    if (m->dtype != RN_DTYPE_F32 && mode != RN_FWD_FUSED) return RN_ERR_UNSUPPORTED;
    if (!default_size(m)) return images_need_default(m);
    if (B > m->crops_cap) {
        if (m->crops_cap > 0 && rn_ctx_graphs_live(m->ctx) > 0) return RN_ERR_INVALID;
        if (m->crops) TRY(rn_free(m->ctx, m->crops));
        m->crops = NULL;
        m->crops_cap = 0;
        TRY(rn_malloc(m->ctx, (void **)&m->crops, B * 3 * RN_DEFAULT_SIDE * RN_DEFAULT_SIDE));
        m->crops_cap = B;
    }
    run_begin(m, m->ctx, 0, 0, mode);
    m->n_prof = 0;
    TRY(prof_begin(m, "image_u8_resize_crop", "input", 0.0,
                   src_bytes + (double)B * 3.0 * RN_DEFAULT_SIDE * RN_DEFAULT_SIDE));
    TRY(rn_image_u8_resize_crop_launch(m->ctx, packed_dev, table_dev, B, m->crops, RN_DEFAULT_SIDE));
    TRY(prof_end(m));
    return forward_any(m, m->crops, 1, B, logits, mode, 1); /* keeps the resize launch's record */
}

int rn_model_forward_images_u8(rn_model *m, const uint8_t *packed_dev, const uint64_t *offsets,
                               const uint64_t *heights, const uint64_t *widths, uint64_t B, float *logits, int mode)
{
    const double crop = (double)RN_DEFAULT_SIDE / RN_RESIZE_SIDE;
    uint64_t bytes = 0, i;
    double src_bytes = 0.0;
    void *host, *dev = NULL;
    int st;
    if (!m || !packed_dev || !offsets || !heights || !widths || !logits || B == 0) return RN_ERR_INVALID;
    if (!default_size(m)) return images_need_default(m);
    if (rn_image_u8_resize_crop_table(offsets, heights, widths, B, RN_RESIZE_SIDE, RN_DEFAULT_SIDE, NULL, 0, &bytes) !=
        RN_OK)
        return RN_ERR_INVALID;
    if (rn_ctx_is_capturing(m->ctx)) return RN_ERR_UNSUPPORTED; /* the tables come from host memory freed below */
    host = malloc(bytes);
    if (!host) return RN_ERR_NOMEM;
    st = rn_image_u8_resize_crop_table(offsets, heights, widths, B, RN_RESIZE_SIDE, RN_DEFAULT_SIDE, host, bytes, &bytes);
    if (st == RN_OK) st = rn_ctx_scratch_slot(m->ctx, 5, bytes, &dev);
    if (st == RN_OK) st = rn_ctx_upload_sync(m->ctx, dev, host, bytes);
    free(host);
    if (st != RN_OK) return st;
    for (i = 0; i < B; ++i) src_bytes += 3.0 * (double)heights[i] * (double)widths[i] * crop * crop;
    return rn_model_forward_images_table(m, packed_dev, dev, B, src_bytes, logits, mode);
}

#define RN_TUNE_ROUNDS 6

/* time every tile candidate of every contraction of a forward of B images (one launch batch);
 * the winners go to slot `slot` of the layers' tile tables */
static int tune_at(rn_model *m, const float *input_nchw, uint64_t B, float *logits, int mode, int slot)
{
    rn_event *e0 = NULL, *e1 = NULL;
    const int ncand = rn_conv_tile_candidates();
    float cand_ms[64];
    int i, c, r, st;
    if (ncand + 1 > 64) return RN_ERR_INVALID;
    m->single_stream_only = 1;
    /* one recorded forward with the per-launch choice: fills the buffers with real data */
    m->n_calls = 0;
    m->recording = 1;
    st = rn_model_forward(m, input_nchw, B, logits, mode);
    m->recording = 0;
    m->single_stream_only = 0;
    if (st != RN_OK) return st;
    st = rn_event_create(m->ctx, &e0);
    if (st == RN_OK) st = rn_event_create(m->ctx, &e1);
    for (i = 0; st == RN_OK && i < m->n_calls; ++i) {
        const rn_conv_call *k = &m->calls[i];
        rn_conv *cv = &m->convs[k->conv];
        float best = 1e30f;
        int best_c = 0, seen = 0, j;
        for (j = 0; j < i; ++j) /* the slices of a depth-first front repeat their calls */
            seen |= m->calls[j].conv == k->conv && m->calls[j].pair_block == k->pair_block &&
                    m->calls[j].B == k->B;
        if (seen) continue;
        /* repetitions outside, candidates inside: a clock or temperature drift during the
         * measurement meets every candidate alike (candidate by candidate, the later ones were
         * timed on a warmer chip); the first round warms the caches and is not counted */
        for (c = 0; c <= ncand; ++c) cand_ms[c] = 1e30f;
        for (r = 0; r < RN_TUNE_ROUNDS && st == RN_OK; ++r) {
            for (c = 0; c <= ncand && st == RN_OK; ++c) { /* 0 = the per-launch choice itself */
                float t = 0.f;
                rn_ctx_set_conv_tile(m->ctx, c);
                st = rn_event_record(m->ctx, e0);
                if (st == RN_OK) st = launch_call(m, m->ctx, k);
                if (st == RN_OK) st = rn_event_record(m->ctx, e1);
                if (st == RN_OK) st = rn_event_elapsed_ms(e0, e1, &t);
                if (r > 0 && t < cand_ms[c]) cand_ms[c] = t;
            }
        }
        for (c = 0; c <= ncand; ++c) {
            if (cand_ms[c] < best * 0.995f) { /* ties keep the earlier (default) candidate */
                best = cand_ms[c];
                best_c = c;
            }
        }
        if (k->pair_block >= 0) {
            m->blocks[k->pair_block].pair_tile[slot] = best_c;
            m->blocks[k->pair_block].pair_tile_B[slot] = k->B;
        } else {
            cv->tile[slot] = best_c;
            cv->tile_B[slot] = k->B;
        }
    }
    rn_ctx_set_conv_tile(m->ctx, 0);
    rn_event_destroy(e0);
    rn_event_destroy(e1);
    return st;
}

int rn_model_tune(rn_model *m, const float *input_nchw, uint64_t B, float *logits, int mode)
{
    const uint64_t B_all = B;
    uint64_t Bp;
    int c, st;
    if (!m) return RN_ERR_INVALID;
    if (B > m->max_sub) B = m->max_sub; /* the launches of a larger batch are sub-batches */
    Bp = B;
    {   /* ... and those run as `streams` parts */
        const int parts = parts_of(m, B);
        if (parts > 1) Bp = B / (uint64_t)parts;
    }
    m->tuned_B = 0;
    for (c = 0; c < m->n_convs; ++c) m->convs[c].tile_B[0] = m->convs[c].tile_B[1] = 0;
    for (c = 0; c < m->n_blocks; ++c) m->blocks[c].pair_tile_B[0] = m->blocks[c].pair_tile_B[1] = 0;
    st = tune_at(m, input_nchw, Bp, logits, mode, 0);
    /* the whole (sub-)batch on one stream is what a profiled forward launches: its own tiles */
    if (st == RN_OK && Bp != B) st = tune_at(m, input_nchw, B, logits, mode, 1);
    if (st != RN_OK) return st;
    m->tuned_B = B;
    m->tuned_mode = mode;
    /* leave the buffers and the logits as a normal forward would */
    return rn_model_forward(m, input_nchw, B_all, logits, mode);
}

/* ---- tuned tiles as data ----------------------------------------------------------------
 * The table rn_model_tune fills, as words: a header that names what it was measured for, then
 * per convolution and per fused pair the two (tile, launch batch) slots.  A model of the same
 * architecture, element type and fusion settings on an identical device takes it over instead of
 * timing every candidate again: the shards of a node (rn_shard_tune tunes ONE shard), or a later
 * process.  Tiles only change speed, never bits, so a stale table costs time, not parity. */
#define RN_TUNING_MAGIC 0x726e54554e453034ull /* "rnTUNE04" */
#define RN_TUNING_HEADER 10 /* of a 224 x 224 model; a model of another size appends tuning_size */

/* header word 9: 0 for the plain (1, 64) networks, whose tables keep their format */
static uint64_t tuning_family(const rn_model *m)
{
    return m->groups == 1 && m->width_per_group == 64 ? 0 : (uint64_t)m->groups << 32 | (uint64_t)m->width_per_group;
}

/* header word 10, present only when not 0: 0 for 224 x 224 models, whose tables keep their format.  A table and
 * a model of different sizes differ in this word or in the table's length. */
static uint64_t tuning_size(const rn_model *m)
{
    return m->H == RN_DEFAULT_SIDE && m->W == RN_DEFAULT_SIDE ? 0 : m->H << 32 | m->W;
}

/* the header word behind those, present only when not 0: 0 for undilated models, whose tables keep their format.
 * The tag in its top byte is one no size word has (sides are at most 2048), so a table of a sized model and one of
 * a dilated model of the same length still differ. */
static uint64_t tuning_dilation(const rn_model *m)
{
    const uint64_t flags = (uint64_t)(m->dilate[0] | m->dilate[1] << 1 | m->dilate[2] << 2);
    return flags ? 0xD1ull << 56 | flags : 0;
}

static uint64_t tuning_header(const rn_model *m)
{
    return RN_TUNING_HEADER + (tuning_size(m) ? 1 : 0) + (tuning_dilation(m) ? 1 : 0);
}

static uint64_t tuning_settings(const rn_model *m)
{
    return (uint64_t)m->pair_fusion | (uint64_t)m->stem_exact << 1 | (uint64_t)m->stem_pool << 2 |
           (uint64_t)m->chain << 4 | (uint64_t)m->front_parts << 8;
}

int rn_model_export_tuning(const rn_model *m, uint64_t *words, uint64_t cap, uint64_t *n_words)
{
    uint64_t need, at = 0;
    int c, k;
    if (!m || !n_words) return RN_ERR_INVALID;
    need = tuning_header(m) + 4 * ((uint64_t)m->n_convs + (uint64_t)m->n_blocks);
    *n_words = need;
    if (!words) return RN_OK; /* size query */
    if (cap < need || !m->tuned_B) return RN_ERR_INVALID;
    words[at++] = RN_TUNING_MAGIC;
    words[at++] = (uint64_t)m->arch;
    words[at++] = (uint64_t)m->dtype;
    words[at++] = tuning_settings(m);
    words[at++] = m->tuned_B;
    words[at++] = (uint64_t)m->tuned_mode;
    words[at++] = (uint64_t)m->n_convs;
    words[at++] = (uint64_t)m->n_blocks;
    words[at++] = (uint64_t)rn_conv_tile_candidates();
    words[at++] = tuning_family(m);
    if (tuning_size(m)) words[at++] = tuning_size(m);
    if (tuning_dilation(m)) words[at++] = tuning_dilation(m);
    for (c = 0; c < m->n_convs; ++c)
        for (k = 0; k < 2; ++k) {
            words[at++] = (uint64_t)m->convs[c].tile[k];
            words[at++] = m->convs[c].tile_B[k];
        }
    for (c = 0; c < m->n_blocks; ++c)
        for (k = 0; k < 2; ++k) {
            words[at++] = (uint64_t)m->blocks[c].pair_tile[k];
            words[at++] = m->blocks[c].pair_tile_B[k];
        }
    return RN_OK;
}

int rn_model_import_tuning(rn_model *m, const uint64_t *words, uint64_t n_words)
{
    uint64_t at;
    int c, k;
    if (!m || !words || n_words < tuning_header(m)) return RN_ERR_INVALID;
    at = tuning_header(m);
    if (words[0] != RN_TUNING_MAGIC || words[1] != (uint64_t)m->arch || words[2] != (uint64_t)m->dtype ||
        words[3] != tuning_settings(m) || words[6] != (uint64_t)m->n_convs || words[7] != (uint64_t)m->n_blocks ||
        words[8] != (uint64_t)rn_conv_tile_candidates() || words[9] != tuning_family(m) ||
        (tuning_size(m) && words[RN_TUNING_HEADER] != tuning_size(m)) ||
        (tuning_dilation(m) && words[at - 1] != tuning_dilation(m)) ||
        n_words != at + 4 * ((uint64_t)m->n_convs + (uint64_t)m->n_blocks))
        return RN_ERR_INVALID; /* measured for another model, size, dilation, setting or build */
    for (c = 0; c < m->n_convs + m->n_blocks; ++c) /* a candidate this build does not have */
        if (words[at + 4 * (uint64_t)c] > (uint64_t)rn_conv_tile_candidates() ||
            words[at + 4 * (uint64_t)c + 2] > (uint64_t)rn_conv_tile_candidates())
            return RN_ERR_INVALID;
    for (c = 0; c < m->n_convs; ++c)
        for (k = 0; k < 2; ++k) {
            m->convs[c].tile[k] = (int)words[at++];
            m->convs[c].tile_B[k] = words[at++];
        }
    for (c = 0; c < m->n_blocks; ++c)
        for (k = 0; k < 2; ++k) {
            m->blocks[c].pair_tile[k] = (int)words[at++];
            m->blocks[c].pair_tile_B[k] = words[at++];
        }
    m->tuned_B = words[4];
    m->tuned_mode = (int)words[5];
    return RN_OK;
}
