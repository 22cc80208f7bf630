// Host pipeline: pinned staging, a copy stream, two slots.  The reference uploads one image,
// runs the forward and downloads the logits strictly in sequence with a device
// synchronisation between every step (main.cu:236-240, tensor.cuh:184-199); at 13k images/s a
// 154 MB batch upload (2.4 ms on PCIe Gen5 x16) would cost 13 % if it were not overlapped.
#include <sched.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "rn_internal.h"
#include "rn_private.h"
#include "rn_resize.h"

struct rn_graph {
    rn_ctx *ctx;
    rn_model *model;  // counted in the model: rn_model_destroy refuses while a graph of it lives
    rn_ctx *pinned[8];  // every context the model queued batch parts on: pinned while the graph lives
    int n_pinned;
    hipGraph_t graph;
    hipGraphExec_t exec;
    size_t nodes;
};

struct rn_pipeline_slot {
    void *h_in, *d_in;  // pinned staging and device input: fp32 NCHW, or 8-bit RGB in a byte pipeline
    float *h_out, *d_out;
    uint64_t *h_idx, *d_idx;  // class indices (first maximum wins, main.cu:243-249)
    uint64_t n;               // images of the batch in this slot (<= B)
    hipEvent_t uploaded, done;
    int busy;
};

struct rn_pipeline {
    rn_model *model;
    void *model_cell;  // rn_model_pipeline_attach: the model counts this pipeline (its buffers are sized for the model's input)
    rn_ctx *ctx;
    uint64_t B;
    uint64_t classes;  // the model's class count when the pipeline was created: the row length of d_out / h_out
    int mode;
    int u8;            // input format: 0 = fp32 NCHW, 1 = 8-bit RGB [B,H,W,3] (rn_pipeline_create_u8),
                       // 2 = decoded 8-bit RGB images of any size (rn_pipeline_create_images_u8)
    size_t img_bytes;  // of one image in that format (formats 0 and 1)
    size_t max_bytes;  // format 2: pixels of one batch; the tables sit at table_off = max_bytes rounded up to 16
    size_t table_off, table_room;
    hipStream_t copy_stream;
    int copy_threads;  // helper threads of the pageable -> pinned copy (RN_COPY_THREADS, default 3)
    rn_pipeline_slot slot[2];
    uint64_t head, tail;  // submitted / collected counts
};

extern "C" {

int rn_graph_destroy(rn_graph *g)
{
    if (!g) return RN_OK;
    if (g->ctx) (void)hipStreamSynchronize(g->ctx->stream);
    if (g->exec) {
        (void)hipGraphExecDestroy(g->exec);
        // the pinned contexts are alive: those of the model's extra streams belong to the model, and
        // the model cannot be destroyed while this graph is counted in it
        for (int i = 0; i < g->n_pinned; ++i) --g->pinned[i]->graphs_live;
        if (g->n_pinned) rn_model_graph_ref(g->model, -1);
    }
    if (g->graph) (void)hipGraphDestroy(g->graph);
    free(g);
    return RN_OK;
}

int rn_model_capture(rn_model *m, const float *input_nchw, uint64_t B, float *logits, int mode,
                     rn_graph **out)
{
    if (!m || !out) return RN_ERR_INVALID;
    *out = nullptr;
    rn_ctx *ctx = rn_model_context(m);
    RN_TRY(rn_bind_device(ctx));
    if (ctx->sync_each_op)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_model_capture: sync_each_op must be off");
    if (rn_model_profiling_enabled(m))
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_model_capture: profiling must be off");
    // eager pass: validates the arguments, sizes the arenas and the scratch outside the capture
    RN_TRY(rn_model_forward(m, input_nchw, B, logits, mode));
    RN_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    rn_graph *g = (rn_graph *)calloc(1, sizeof(rn_graph));
    if (!g) return RN_ERR_NOMEM;
    g->ctx = ctx;
    hipError_t e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) {
        free(g);
        return rn_check_hip(ctx, e, "hipStreamBeginCapture");
    }
    const int st = rn_model_forward(m, input_nchw, B, logits, mode);
    e = hipStreamEndCapture(ctx->stream, &g->graph);  // always end the capture, even on error
    if (st != RN_OK || e != hipSuccess) {
        rn_graph_destroy(g);
        return st != RN_OK ? st : rn_check_hip(ctx, e, "hipStreamEndCapture");
    }
    e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        g->exec = nullptr;
        rn_graph_destroy(g);
        return rn_check_hip(ctx, e, "hipGraphInstantiate");
    }
    // from here on the scratch and the arenas must stay where they are: the captured nodes point
    // into the scratch of the primary context AND of the contexts of the other batch parts
    g->n_pinned = rn_model_contexts(m, g->pinned, 8);
    for (int i = 0; i < g->n_pinned; ++i) ++g->pinned[i]->graphs_live;
    g->model = m;
    rn_model_graph_ref(m, +1);
    e = hipGraphGetNodes(g->graph, nullptr, &g->nodes);
    if (e != hipSuccess) {
        rn_graph_destroy(g);
        return rn_check_hip(ctx, e, "hipGraphGetNodes");
    }
    *out = g;
    return RN_OK;
}

int rn_graph_launch(rn_graph *g)
{
    if (!g) return RN_ERR_INVALID;
    RN_TRY(rn_bind_device(g->ctx));
    RN_HIP_TRY(g->ctx, hipGraphLaunch(g->exec, g->ctx->stream));
    return RN_OK;
}

uint64_t rn_graph_node_count(const rn_graph *g) { return g ? (uint64_t)g->nodes : 0; }

int rn_pipeline_destroy(rn_pipeline *p)
{
    if (!p) return RN_OK;
    if (p->ctx) (void)hipSetDevice(p->ctx->device);
    if (p->ctx) (void)hipStreamSynchronize(p->ctx->stream);
    if (p->copy_stream) (void)hipStreamSynchronize(p->copy_stream);
    for (int i = 0; i < 2; ++i) {
        rn_pipeline_slot *s = &p->slot[i];
        if (s->h_in) (void)hipHostFree(s->h_in);
        if (s->h_out) (void)hipHostFree(s->h_out);
        if (s->h_idx) (void)hipHostFree(s->h_idx);
        if (s->d_in) (void)hipFree(s->d_in);
        if (s->d_out) (void)hipFree(s->d_out);
        if (s->d_idx) (void)hipFree(s->d_idx);
        if (s->uploaded) (void)hipEventDestroy(s->uploaded);
        if (s->done) (void)hipEventDestroy(s->done);
    }
    if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
    rn_model_pipeline_detach(p->model_cell);
    free(p);
    return RN_OK;
}

static int pipeline_create(rn_model *m, rn_pipeline **out, uint64_t B, int mode, int u8, uint64_t max_batch_bytes = 0)
{
    if (!m || !out || B == 0 || (u8 == 2 && max_batch_bytes == 0)) return RN_ERR_INVALID;
    *out = nullptr;
    rn_ctx *ctx = rn_model_context(m);
    uint64_t H = 0, W = 0;
    rn_model_input_size(m, &H, &W);
    if (u8 == 2 && (H != 224 || W != 224))
        return rn_set_error(ctx, RN_ERR_UNSUPPORTED, "rn_pipeline_create_images_u8: decoded images are resized to 256 and "
                            "cropped to 224 x 224; the model's input size is %llu x %llu",
                            (unsigned long long)H, (unsigned long long)W);
    rn_pipeline *p = (rn_pipeline *)calloc(1, sizeof(rn_pipeline));
    if (!p) return RN_ERR_NOMEM;
    p->model = m;
    p->model_cell = rn_model_pipeline_attach(m);
    p->ctx = ctx;
    p->B = B;
    p->classes = rn_model_classes(m);
    p->mode = mode;
    p->u8 = u8;
    p->img_bytes = (size_t)(3 * H * W) * (u8 ? sizeof(uint8_t) : sizeof(float));  // the model's size now: it stays while this pipeline lives
    {
        const char *ct = getenv("RN_COPY_THREADS");
        const int n = ct ? atoi(ct) : 3;
        p->copy_threads = n < 1 ? 1 : n > 16 ? 16 : n;
    }
    // format 2: behind the pixels the tables.  One image's table is 12 descriptor words plus, per axis, 224 x
    // (2 + ksize) words with ksize <= 2 * scale + 3; its pixels are at least 3 * (256 * scale)^2 bytes, so
    // everything a table holds beyond the scale-1 size (12,544 bytes) is less than 1/16 of the batch's pixels
    p->max_bytes = (size_t)max_batch_bytes;
    p->table_off = ((size_t)max_batch_bytes + 15) & ~(size_t)15;
    p->table_room = (size_t)B * (RN_RS_DESC * 4 + 12544) + (size_t)max_batch_bytes / 16 + 64;
    const size_t in_bytes = u8 == 2 ? p->table_off + p->table_room : (size_t)B * p->img_bytes;
    const size_t out_bytes = (size_t)B * p->classes * sizeof(float);
    const size_t idx_bytes = (size_t)B * sizeof(uint64_t);
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        rn_pipeline_slot *s = &p->slot[i];
        e = hipHostMalloc(&s->h_in, in_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_out, out_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&s->h_idx, idx_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipMalloc(&s->d_in, in_bytes);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_out, out_bytes);
        if (e == hipSuccess) e = hipMalloc((void **)&s->d_idx, idx_bytes);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->uploaded, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s->done, hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        const int st = rn_check_hip(ctx, e, "rn_pipeline_create");
        rn_pipeline_destroy(p);
        return st;
    }
    *out = p;
    return RN_OK;
}

int rn_pipeline_create(rn_model *m, rn_pipeline **out, uint64_t B, int mode)
{
    return pipeline_create(m, out, B, mode, 0);
}

int rn_pipeline_create_u8(rn_model *m, rn_pipeline **out, uint64_t B, int mode)
{
    return pipeline_create(m, out, B, mode, 1);
}

int rn_pipeline_create_images_u8(rn_model *m, rn_pipeline **out, uint64_t B, int mode, uint64_t max_batch_bytes)
{
    return pipeline_create(m, out, B, mode, 2, max_batch_bytes);
}

uint64_t rn_pipeline_in_flight(const rn_pipeline *p) { return p ? p->head - p->tail : 0; }
uint64_t rn_pipeline_batch(const rn_pipeline *p) { return p ? p->B : 0; }

// a float call on a byte pipeline or the reverse
static int wrong_format(rn_pipeline *p, const char *who)
{
    return rn_set_error(p->ctx, RN_ERR_INVALID, "%s: the pipeline was created for %s input", who,
                        p->u8 == 2   ? "decoded images (rn_pipeline_create_images_u8)"
                        : p->u8 == 1 ? "8-bit RGB (rn_pipeline_create_u8)"
                                     : "fp32 NCHW (rn_pipeline_create)");
}

static int input_buffer(rn_pipeline *p, void **host_staging, int u8, const char *who)
{
    if (!p || !host_staging) return RN_ERR_INVALID;
    if (p->u8 != u8) return wrong_format(p, who);
    if (p->head - p->tail >= 2)
        return rn_set_error(p->ctx, RN_ERR_INVALID, "%s: both slots busy, collect first", who);
    *host_staging = p->slot[p->head & 1].h_in;
    return RN_OK;
}

int rn_pipeline_input_buffer(rn_pipeline *p, float **host_staging)
{
    return input_buffer(p, (void **)host_staging, 0, "rn_pipeline_input_buffer");
}

int rn_pipeline_input_buffer_u8(rn_pipeline *p, uint8_t **host_staging)
{
    return input_buffer(p, (void **)host_staging, 1, "rn_pipeline_input_buffer_u8");
}

// host_input: n images in the pipeline's input format
static int submit_n(rn_pipeline *p, const void *host_input, uint64_t n, int u8, const char *who)
{
    if (!p) return RN_ERR_INVALID;
    rn_ctx *ctx = p->ctx;
    RN_TRY(rn_bind_device(ctx));
    if (p->u8 != u8) return wrong_format(p, who);
    if (n == 0 || n > p->B)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_submit_n: %llu images, the pipeline holds 1..%llu",
                            (unsigned long long)n, (unsigned long long)p->B);
    if (p->head - p->tail >= 2)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_submit: both slots busy, collect first");
    rn_pipeline_slot *s = &p->slot[p->head & 1];
    const size_t in_bytes = (size_t)n * p->img_bytes;
    const int st = [&]() -> int {
        if (host_input && host_input != s->h_in) {
            // pageable -> pinned -> device in pieces of 16 images (at 224 x 224 9.6 MB of fp32, 2.4 MB of bytes): the upload of piece i runs on the
            // copy stream while piece i+1 is being copied, so a batch costs max(copy, upload) instead of their
            // sum before its forward can start.  One core copies a 154 MB fp32 batch in 6-7 ms (23 GB/s), which
            // is longer than its upload (3.8 ms) and than a bf16 forward (3.3 ms): the pieces are copied by
            // `copiers` helper threads (they inherit this thread's CPU affinity: the cores local to the device)
            // while this thread queues each piece's upload as soon as it has landed in staging.
            const size_t piece = (size_t)16 * p->img_bytes;
            const size_t npieces = (in_bytes + piece - 1) / piece;
            const int copiers = npieces >= 4 ? p->copy_threads : 1;
            auto copy_piece = [&](size_t i) {
                const size_t at = i * piece, nb = in_bytes - at < piece ? in_bytes - at : piece;
                memcpy((char *)s->h_in + at, (const char *)host_input + at, nb);
            };
            auto upload_piece = [&](size_t i) -> hipError_t {
                const size_t at = i * piece, nb = in_bytes - at < piece ? in_bytes - at : piece;
                return hipMemcpyAsync((char *)s->d_in + at, (char *)s->h_in + at, nb, hipMemcpyHostToDevice, p->copy_stream);
            };
            if (copiers <= 1) {
                for (size_t i = 0; i < npieces; ++i) {
                    copy_piece(i);
                    RN_HIP_TRY(ctx, upload_piece(i));
                }
            } else {
                std::vector<std::atomic<int>> landed(npieces);
                for (auto &f : landed) f.store(0, std::memory_order_relaxed);
                std::vector<std::thread> pool;
                int started = 0;  // a thread that cannot be created leaves its pieces to this thread
                try {
                    for (int t = 0; t < copiers; ++t) {
                        pool.emplace_back([&, t]() {
                            for (size_t i = (size_t)t; i < npieces; i += (size_t)copiers) {
                                copy_piece(i);
                                landed[i].store(1, std::memory_order_release);
                            }
                        });
                        ++started;
                    }
                } catch (...) {
                }
                hipError_t e = hipSuccess;
                for (size_t i = 0; i < npieces && e == hipSuccess; ++i) {
                    if ((int)(i % (size_t)copiers) >= started)
                        copy_piece(i);
                    else
                        while (!landed[i].load(std::memory_order_acquire)) sched_yield();
                    e = upload_piece(i);
                }
                for (auto &th : pool) th.join();  // also on an error: the threads write into the slot's staging
                RN_HIP_TRY(ctx, e);
            }
        } else {
            RN_HIP_TRY(ctx, hipMemcpyAsync(s->d_in, s->h_in, in_bytes, hipMemcpyHostToDevice, p->copy_stream));
        }
        RN_HIP_TRY(ctx, hipEventRecord(s->uploaded, p->copy_stream));
        // forward on the compute stream once the upload has landed; the other slot's forward may
        // still be running there, which is exactly the overlap
        RN_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s->uploaded, 0));
        if (p->u8)
            RN_TRY(rn_model_forward_u8(p->model, (const uint8_t *)s->d_in, n, s->d_out, p->mode));
        else
            RN_TRY(rn_model_forward(p->model, (const float *)s->d_in, n, s->d_out, p->mode));
        RN_TRY(rn_argmax_forward(ctx, s->d_out, s->d_idx, n, p->classes));
        RN_HIP_TRY(ctx, hipMemcpyAsync(s->h_out, s->d_out, (size_t)n * p->classes * sizeof(float), hipMemcpyDeviceToHost,
                                       ctx->stream));
        RN_HIP_TRY(ctx, hipMemcpyAsync(s->h_idx, s->d_idx, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                       ctx->stream));
        RN_HIP_TRY(ctx, hipEventRecord(s->done, ctx->stream));
        return RN_OK;
    }();
    if (st != RN_OK) {
        // the slot stays free, so the next submit writes its staging buffer again: whatever part of
        // this batch was queued (the upload reads h_in) has to be over before that
        (void)hipStreamSynchronize(p->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        return st;
    }
    s->busy = 1;
    s->n = n;
    ++p->head;
    return RN_OK;
}

int rn_pipeline_submit_n(rn_pipeline *p, const float *host_input_nchw, uint64_t n)
{
    return submit_n(p, host_input_nchw, n, 0, "rn_pipeline_submit_n");
}

int rn_pipeline_submit_u8_n(rn_pipeline *p, const uint8_t *host_input_nhwc, uint64_t n)
{
    return submit_n(p, host_input_nhwc, n, 1, "rn_pipeline_submit_u8_n");
}

int rn_pipeline_submit_images_u8_n(rn_pipeline *p, const uint8_t *const *host_imgs, const uint64_t *heights,
                                   const uint64_t *widths, uint64_t n)
{
    if (!p) return RN_ERR_INVALID;
    rn_ctx *ctx = p->ctx;
    RN_TRY(rn_bind_device(ctx));
    if (p->u8 != 2) return wrong_format(p, "rn_pipeline_submit_images_u8_n");
    if (!host_imgs || !heights || !widths) return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_submit_images_u8_n: null pointer");
    if (n == 0 || n > p->B)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_submit_images_u8_n: %llu images, the pipeline holds 1..%llu",
                            (unsigned long long)n, (unsigned long long)p->B);
    if (p->head - p->tail >= 2)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_submit_images_u8_n: both slots busy, collect first");
    std::vector<uint64_t> offs(n);
    uint64_t total = 0, tbytes = 0;
    double src_bytes = 0.0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!host_imgs[i] || heights[i] > RN_RS_MAX_SIDE || widths[i] > RN_RS_MAX_SIDE)
            return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_submit_images_u8_n: image %llu: null or too large", (unsigned long long)i);
        offs[i] = total;
        total += heights[i] * widths[i] * 3;
        src_bytes += 3.0 * (double)heights[i] * (double)widths[i] * (224.0 / 256.0) * (224.0 / 256.0);
    }
    if (total > p->max_bytes)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_submit_images_u8_n: the batch holds %llu bytes, the pipeline was "
                            "created for %llu (max_batch_bytes)", (unsigned long long)total, (unsigned long long)p->max_bytes);
    rn_pipeline_slot *s = &p->slot[p->head & 1];
    char *tab = (char *)s->h_in + p->table_off;
    if (rn_image_u8_resize_crop_table(offs.data(), heights, widths, n, 256, 224, tab, p->table_room, &tbytes) != RN_OK)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_submit_images_u8_n: an image the resize refuses (sides 1..16384, "
                            "at most 64 times their resized length)");
    const int st = [&]() -> int {
        // pageable -> pinned: the images are dealt to the helper threads, this thread takes its share
        const int copiers = n >= 4 ? p->copy_threads : 1;
        auto copy_share = [&](int t) {
            for (uint64_t i = (uint64_t)t; i < n; i += (uint64_t)copiers)
                memcpy((char *)s->h_in + offs[i], host_imgs[i], (size_t)(heights[i] * widths[i] * 3));
        };
        std::vector<std::thread> pool;
        int started = 1;
        try {
            for (int t = 1; t < copiers; ++t) {
                pool.emplace_back(copy_share, t);
                ++started;
            }
        } catch (...) {
        }
        copy_share(0);
        for (auto &th : pool) th.join();
        for (int t = started; t < copiers; ++t) copy_share(t);
        RN_HIP_TRY(ctx, hipMemcpyAsync(s->d_in, s->h_in, (size_t)total, hipMemcpyHostToDevice, p->copy_stream));
        RN_HIP_TRY(ctx, hipMemcpyAsync((char *)s->d_in + p->table_off, tab, (size_t)tbytes, hipMemcpyHostToDevice, p->copy_stream));
        RN_HIP_TRY(ctx, hipEventRecord(s->uploaded, p->copy_stream));
        RN_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, s->uploaded, 0));
        RN_TRY(rn_model_forward_images_table(p->model, (const uint8_t *)s->d_in, (char *)s->d_in + p->table_off, n, src_bytes,
                                             s->d_out, p->mode));
        RN_TRY(rn_argmax_forward(ctx, s->d_out, s->d_idx, n, p->classes));
        RN_HIP_TRY(ctx, hipMemcpyAsync(s->h_out, s->d_out, (size_t)n * p->classes * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        RN_HIP_TRY(ctx, hipMemcpyAsync(s->h_idx, s->d_idx, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        RN_HIP_TRY(ctx, hipEventRecord(s->done, ctx->stream));
        return RN_OK;
    }();
    if (st != RN_OK) {
        (void)hipStreamSynchronize(p->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        return st;
    }
    s->busy = 1;
    s->n = n;
    ++p->head;
    return RN_OK;
}

int rn_pipeline_submit(rn_pipeline *p, const float *host_input_nchw)
{
    return p ? rn_pipeline_submit_n(p, host_input_nchw, p->B) : RN_ERR_INVALID;
}

int rn_pipeline_collect_n(rn_pipeline *p, float *host_logits, uint64_t *host_top1, uint64_t *n)
{
    if (!p) return RN_ERR_INVALID;
    rn_ctx *ctx = p->ctx;
    if (p->head == p->tail)
        return rn_set_error(ctx, RN_ERR_INVALID, "rn_pipeline_collect: nothing in flight");
    rn_pipeline_slot *s = &p->slot[p->tail & 1];
    RN_TRY(rn_bind_device(ctx));
    RN_HIP_TRY(ctx, hipEventSynchronize(s->done));
    if (host_logits) memcpy(host_logits, s->h_out, (size_t)s->n * p->classes * sizeof(float));
    if (host_top1) memcpy(host_top1, s->h_idx, (size_t)s->n * sizeof(uint64_t));
    if (n) *n = s->n;
    s->busy = 0;
    ++p->tail;
    return RN_OK;
}

int rn_pipeline_collect(rn_pipeline *p, float *host_logits)
{
    if (!p || !host_logits) return RN_ERR_INVALID;
    return rn_pipeline_collect_n(p, host_logits, nullptr, nullptr);
}

}  // extern "C"
