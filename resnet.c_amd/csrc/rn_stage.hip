// What the objects behind the backbone share (rn_private.h, "rn_stage.hip"): the front of set_tensor and finalize over
// a parameter table, the pack of a convolution unit, the side-by-side panel, the scratch growth guard and the frees.
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

}  // extern "C"
