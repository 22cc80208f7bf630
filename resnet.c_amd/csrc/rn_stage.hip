// What the objects behind the backbone share (rn_private.h, "rn_stage.hip"): the front of set_tensor and finalize over
// a parameter table, the pack of a convolution unit, the side-by-side panel, the scratch growth guard and the frees; and
// the RoI tower the mask head and the keypoint head stand on.
// Host code and calls into the library's own entry points: no kernel is defined or launched from here.
#include <stdlib.h>
#include <string.h>

#include "rn_internal.h"
#include "rn_private.h"

extern "C" {

int rn_stage_set_tensor(rn_ctx *ctx, const char *fn, const char *what, int finalized, rn_params *t, const char *key,
                        const float *host_data, uint64_t numel)
{
    if (!ctx) return RN_ERR_INVALID;
    if (!key || !host_data) return rn_set_error(ctx, RN_ERR_INVALID, "%s: key or host_data is NULL", fn);
    if (finalized) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s is finalized", fn, what);
    const int i = rn_params_find(t, key);
    if (i < 0) return rn_set_error(ctx, RN_ERR_INVALID, "%s: unknown key '%s'", fn, key);
    uint64_t wanted = 0;
    switch (rn_params_set(t, i, host_data, numel, &wanted)) {
    case 0: return RN_OK;
    case 1:
        return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s has %llu elements, not %llu", fn, key, (unsigned long long)numel,
                            (unsigned long long)wanted);
    default: return rn_set_error(ctx, RN_ERR_NOMEM, "%s: out of host memory", fn);
    }
}

int rn_stage_all_set(rn_ctx *ctx, const char *fn, const rn_params *t)
{
    const int i = rn_params_first_missing(t);
    return i < 0 ? RN_OK : rn_set_error(ctx, RN_ERR_INVALID, "%s: %s is not set", fn, t->p[i].key);
}

void rn_stage_unit_free(rn_ctx *ctx, rn_stage_unit *u)
{
    rn_free_null(ctx, &u->packed), rn_free_null(ctx, &u->center);
    rn_free_null(ctx, (void **)&u->scale), rn_free_null(ctx, (void **)&u->shift);
}

int rn_stage_pack(rn_ctx *ctx, int dtype, const float *w, uint64_t cin, uint64_t cout, uint64_t k, const float *bias,
                  const float *const *bn, rn_stage_unit *u)
{
    const uint64_t n = cout * cin * k * k * sizeof(float), vec = cout * sizeof(float);
    float *raw = NULL, *stats = NULL;  // the OIHW weight and the batch-norm's four vectors on the device, until packed
    rn_stage_unit_free(ctx, u);
    int st = rn_malloc(ctx, (void **)&raw, n);
    if (st == RN_OK) st = rn_malloc(ctx, &u->packed, rn_conv2d_packed_weight_numel_dt(dtype, cin, cout, k) * rn_elem_size(dtype));
    if (st == RN_OK && (bias || bn)) st = rn_malloc(ctx, (void **)&u->shift, vec);
    if (st == RN_OK && bn) st = rn_malloc(ctx, (void **)&u->scale, vec);
    if (st == RN_OK && bn) st = rn_malloc(ctx, (void **)&stats, 4 * vec);
    if (st == RN_OK) st = rn_ctx_upload_sync(ctx, raw, w, n);
    if (st == RN_OK && bias) st = rn_ctx_upload_sync(ctx, u->shift, bias, vec);
    for (int j = 0; j < 4 && bn && st == RN_OK; ++j) st = rn_ctx_upload_sync(ctx, stats + j * cout, bn[j], vec);
    if (st == RN_OK && bn)
        st = rn_batchnorm2d_fold(ctx, stats, stats + cout, stats + 2 * cout, stats + 3 * cout, u->scale, u->shift, cout);
    if (st == RN_OK) st = rn_conv2d_pack_weight_dt(ctx, dtype, raw, u->packed, cin, cout, k);
    if (st == RN_OK) st = rn_sync(ctx);
    rn_free_null(ctx, (void **)&raw), rn_free_null(ctx, (void **)&stats);
    if (st != RN_OK) rn_stage_unit_free(ctx, u);
    return st;
}

float *rn_stage_side_by_side(const float *wa, const float *ba, uint64_t ra, const float *wb, const float *bb, uint64_t rb,
                             uint64_t len, uint64_t P)
{
    float *w = (float *)calloc(P * len + P, sizeof(float));
    if (!w) return NULL;
    memcpy(w, wa, ra * len * sizeof(float)), memcpy(w + ra * len, wb, rb * len * sizeof(float));
    memcpy(w + P * len, ba, ra * sizeof(float)), memcpy(w + P * len + ra, bb, rb * sizeof(float));
    return w;
}

void rn_stage_free_list(rn_ctx *ctx, const rn_scratch_item *list, int n)
{
    for (int i = 0; i < n; ++i) rn_free_null(ctx, list[i].ptr);
}

int rn_stage_grow(rn_ctx *ctx, const char *who, const rn_scratch_item *list, int n, uint64_t *caps, const uint64_t *want,
                  int n_caps)
{
    bool had = false;
    for (int i = 0; i < n_caps; ++i) had = had || caps[i] > 0;
    if (rn_ctx_is_capturing(ctx))
        return rn_set_error(ctx, RN_ERR_UNSUPPORTED, "%s: the scratch cannot grow on a stream that is being captured", who);
    if (had && ctx->graphs_live > 0)
        return rn_set_error(ctx, RN_ERR_INVALID, "%s: the scratch cannot grow while a captured graph lives", who);
    RN_TRY(rn_sync(ctx));
    rn_stage_free_list(ctx, list, n);
    memset(caps, 0, (size_t)n_caps * sizeof(*caps));
    for (int i = 0; i < n; ++i)
        if (list[i].bytes) RN_TRY(rn_malloc(ctx, list[i].ptr, list[i].bytes));
    memcpy(caps, want, (size_t)n_caps * sizeof(*caps));
    return RN_OK;
}

// ---- the RoI tower under the mask head and the keypoint head (rn_private.h: rn_roi_tower, rn_roi_head) ----

int rn_roi_tower_check(rn_ctx *ctx, const char *fn, uint64_t in_channels, uint64_t n_layers, const uint64_t *layer_channels,
                       const char *own, uint64_t resolution, uint64_t max_resolution)
{
    const char *why = NULL;
    if (in_channels < 64 || in_channels % 64 != 0 || in_channels > 8192) why = "in_channels must be a multiple of 64 (at most 8192)";
    else if (n_layers < 1 || n_layers > RN_TOWER_MAX_LAYERS) why = "n_layers must be 1..8";
    else if (!layer_channels) why = "layer_channels is NULL";
    for (uint64_t i = 0; i < n_layers && !why; ++i)
        if (layer_channels[i] < 64 || layer_channels[i] % 64 != 0 || layer_channels[i] > 8192)
            why = "every layer's channels must be a multiple of 64 (at most 8192)";
    if (!why) why = own;
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    if (resolution < 1 || resolution > max_resolution)
        return rn_set_error(ctx, RN_ERR_INVALID, "%s: resolution must be 1..%d", fn, (int)max_resolution);
    return RN_OK;
}

void rn_roi_tower_init(rn_roi_tower *t, rn_ctx *ctx, uint64_t in_channels, uint64_t n_layers, const uint64_t *layer_channels,
                       uint64_t resolution, rn_roi_tower_key key_of)
{
    t->ctx = ctx, t->Cin = in_channels, t->n_layers = n_layers, t->M = resolution;
    t->widest = in_channels;
    for (uint64_t i = 0; i < n_layers; ++i) {
        t->ch[i] = layer_channels[i];
        if (t->ch[i] > t->widest) t->widest = t->ch[i];
    }
    t->params.prefix = "roi_heads.";  // every key with or without it
    for (uint64_t i = 0; i < n_layers; ++i)
        for (int j = 0; j < 2; ++j) {
            char key[RN_PARAM_KEY], alt[RN_PARAM_KEY];
            key_of((int)i, j ? "bias" : "weight", key, alt);
            const uint64_t rows = j ? 1 : t->ch[i], len = j ? t->ch[i] : (i == 0 ? t->Cin : t->ch[i - 1]) * 9;
            rn_params_add(&t->params, key, alt[0] ? alt : NULL, rows, len, rows, len, 0.0f);
        }
}

int rn_roi_tower_pack_layers(rn_roi_tower *t, const char *fn)
{
    RN_TRY(rn_stage_all_set(t->ctx, fn, &t->params));
    const rn_params_entry *p = t->params.p;
    for (uint64_t i = 0; i < t->n_layers; ++i)
        RN_TRY(rn_stage_pack(t->ctx, RN_DTYPE_F32, p[2 * i].host, i == 0 ? t->Cin : t->ch[i - 1], t->ch[i], 3, p[2 * i + 1].host, NULL,
                             &t->unit[i]));
    return RN_OK;
}

int rn_roi_tower_pack_panel(rn_roi_tower *t, const float *w, const float *shift)
{
    return rn_stage_pack(t->ctx, RN_DTYPE_F32, w, t->ch[t->n_layers - 1], t->panel, 1, shift, NULL, &t->unit[t->n_layers]);
}

// the scratch tensors for `rows` detections, `pool` of them behind a neck, in the order they are allocated in (a tower
// without the extra tensor asks for no bytes of it)
static void tower_scratch(rn_roi_tower *t, uint64_t rows, uint64_t pool, rn_scratch_item list[RN_TOWER_SCRATCH])
{
    const uint64_t px = rows * t->M * t->M;
    list[0] = {(void **)&t->ping, px * t->widest * sizeof(float)};
    list[1] = {(void **)&t->pong, px * t->widest * sizeof(float)};
    list[2] = {(void **)&t->t, px * t->panel * sizeof(float)};
    list[3] = {(void **)&t->extra, px * t->extra_floats * sizeof(float)};
    list[4] = {(void **)&t->rois, pool * 5 * sizeof(float)};
    list[5] = {(void **)&t->pooled, pool * t->M * t->M * t->Cin * sizeof(float)};
}

void rn_roi_tower_free(rn_roi_tower *t)
{
    rn_scratch_item list[RN_TOWER_SCRATCH];
    tower_scratch(t, 0, 0, list);
    rn_stage_free_list(t->ctx, list, RN_TOWER_SCRATCH);
    rn_params_free(&t->params);
    for (int i = 0; i <= RN_TOWER_MAX_LAYERS; ++i) rn_stage_unit_free(t->ctx, &t->unit[i]);
}

int rn_roi_tower_matches(const rn_roi_tower *t, const rn_ctx *ctx, uint64_t in_channels, const char **why)
{
    const char *w = NULL;
    if (!t) w = "head is NULL";
    else if (!t->finalized) w = "head is not finalized";
    else if (t->ctx->device != ctx->device) w = "head's context is on another device";
    else if (t->Cin != in_channels) w = "head's in_channels is not the neck's out_channels";
    if (why) *why = w;
    return w == NULL;
}

int rn_roi_tower_reserve(rn_roi_tower *t, uint64_t rows, int with_pool)
{
    if (rows <= t->cap[RN_TOWER_ROWS] && (!with_pool || rows <= t->cap[RN_TOWER_POOL])) return RN_OK;
    const uint64_t want[2] = {rows > t->cap[RN_TOWER_ROWS] ? rows : t->cap[RN_TOWER_ROWS],
                              with_pool && rows > t->cap[RN_TOWER_POOL] ? rows : t->cap[RN_TOWER_POOL]};
    rn_scratch_item list[RN_TOWER_SCRATCH];
    tower_scratch(t, want[RN_TOWER_ROWS], want[RN_TOWER_POOL], list);
    return rn_stage_grow(t->ctx, t->name, list, RN_TOWER_SCRATCH, t->cap, want, 2);
}

int rn_roi_head_step(const rn_roi_head *s, rn_ctx *ctx, const float *pooled_nhwc, const int32_t *labels, const float *boxes,
                     uint64_t sub0, uint64_t row0, uint64_t K, uint64_t image_h, uint64_t image_w)
{
    rn_roi_tower *t = s->tower;
    if (sub0 + K > t->cap[RN_TOWER_ROWS]) return rn_set_error(ctx, RN_ERR_INVALID, "%s: scratch not reserved", t->name);
    const uint64_t M = t->M, px0 = sub0 * M * M, n = t->n_layers;
    float *ping = t->ping + px0 * t->widest, *pong = t->pong + px0 * t->widest, *out = t->t + px0 * t->panel;
    rn_epilogue ep;
    ep.scale = NULL, ep.residual = NULL, ep.relu = 1;
    const float *x = pooled_nhwc;
    uint64_t cin = t->Cin;
    for (uint64_t i = 0; i < n; ++i) {
        float *y = i % 2 == 0 ? ping : pong;
        ep.shift = t->unit[i].shift;
        RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, x, y, t->unit[i].packed, 3, 1, 1, M, M, K, cin, t->ch[i], M, M, &ep));
        x = y, cin = t->ch[i];
    }
    ep.shift = t->unit[n].shift, ep.relu = t->panel_relu;
    RN_TRY(rn_conv2d_nhwc_forward_dt(ctx, RN_DTYPE_F32, RN_DTYPE_F32, x, out, t->unit[n].packed, 1, 1, 0, M, M, K, cin, t->panel, M, M, &ep));
    return s->behind(s, ctx, out, t->extra ? t->extra + px0 * t->extra_floats : NULL, labels, boxes, row0, K, image_h, image_w);
}

int rn_roi_head_stage(const rn_roi_head *s, rn_ctx *ctx, const void *const *maps, const uint64_t *hs, const uint64_t *ws,
                      uint64_t images, uint64_t sub0, uint64_t img0, uint64_t B, uint64_t D, const float *boxes,
                      const int32_t *labels, uint64_t image_h, uint64_t image_w)
{
    rn_roi_tower *t = s->tower;
    const rn_roi_pool_view *v = &s->pool;
    const uint64_t M = t->M, K = B * D, row0 = img0 * D, srow0 = sub0 * D, feat = M * M * t->Cin;
    if ((!v->rois || !v->pooled) && srow0 + K > t->cap[RN_TOWER_POOL])
        return rn_set_error(ctx, RN_ERR_INVALID, "%s: scratch not reserved", t->name);
    float *rois = v->rois ? v->rois + row0 * 5 : t->rois + srow0 * 5;
    float *pooled = v->pooled ? v->pooled + row0 * feat : t->pooled + srow0 * feat;
    RN_TRY(rn_detection_rois_window(ctx, boxes + row0 * 4, labels + row0, img0, B, D, rois));
    RN_TRY(rn_roi_align_nhwc_window(ctx, RN_DTYPE_F32, (uint64_t)v->n_levels, maps, hs, ws, s->scales, s->thr, images, img0, B, 1,
                                    t->Cin, rois, K, M, M, v->sampling_ratio, v->aligned, pooled, NULL));
    return rn_roi_head_step(s, ctx, pooled, labels + row0, boxes + row0 * 4, srow0, row0, K, image_h, image_w);
}

int rn_roi_head_forward(const rn_roi_head *s, const char *fn, const float *pooled_nhwc, const char *own, const rn_operand *ops,
                        int n_ops, const int32_t *labels, const float *boxes, uint64_t K, uint64_t image_h, uint64_t image_w)
{
    rn_ctx *ctx = s->tower->ctx;
    const char *why = own;
    if (!pooled_nhwc) why = "pooled_nhwc is NULL";
    else if (!why && (reinterpret_cast<uintptr_t>(pooled_nhwc) & 15) != 0) why = "pooled_nhwc is off a 16-byte boundary";
    if (why) return rn_set_error(ctx, RN_ERR_INVALID, "%s: %s", fn, why);
    RN_TRY(check_operands(ctx, fn, ops, n_ops));
    RN_TRY(rn_roi_tower_reserve(s->tower, K, 0));
    const int saved_layout = ctx->layout;
    ctx->layout = RN_LAYOUT_NHWC;
    const int st = rn_roi_head_step(s, ctx, pooled_nhwc, labels, boxes, 0, 0, K, image_h, image_w);
    ctx->layout = saved_layout;
    return st;
}

}  // extern "C"
