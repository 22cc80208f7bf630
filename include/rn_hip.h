/*
 * rn_hip.h -- C-ABI of the MI355X (gfx950) ResNet forward path.
 *
 * Plain C: pointers, sizes and opaque handles only.  Every entry point returns
 * an int status (RN_OK == 0) and never aborts; rn_last_error() gives the text.
 * Device pointers are ordinary HIP device addresses (hipMalloc / rn_malloc /
 * any framework's allocator on the same device).
 *
 * Each op entry point takes the arguments of the reference kernel it replaces,
 * in the same order, preceded by the context:
 *
 *   rn_conv_output_size      <- convOutputSize            cuda/ops.cuh:9-13
 *   rn_conv2d_forward        <- conv2dForwardKernel       cuda/ops.cuh:15-18  + Conv2d::forward      cuda/nn.cu:3-16
 *   rn_maxpool2d_forward     <- maxPool2dKernel           cuda/ops.cuh:19-21  + Pool2d::maxforward   cuda/nn.cu:43-53
 *   rn_avgpool2d_forward     <- avgPool2dKernel           cuda/ops.cuh:22-24  + Pool2d::avgforward   cuda/nn.cu:31-41
 *   rn_linear_forward        <- linearForwardKernel       cuda/ops.cuh:25-26  + Linear::forward      cuda/nn.cu:55-64
 *   rn_relu_forward          <- reluForwardKernel         cuda/ops.cuh:27     + reluForward          cuda/nn.cu:66-75
 *   rn_batchnorm2d_forward   <- batchNorm2dForwardKernel  cuda/ops.cuh:29-31  + BatchNorm2d::forward cuda/nn.cu:18-29
 *   rn_add_forward           <- addForwardKernel          cuda/ops.cuh:32     + addForward           cuda/nn.cu:77-87
 *
 * Buffers mirror Tensor<T> (cuda/tensor.cuh:59-245):
 *   rn_malloc / rn_free          <- safeCudaMalloc / cudaFree deleter   helpers.cuh:24-35, tensor.cuh:81-86
 *   rn_memcpy_h2d / rn_memcpy_d2h<- Tensor::toDevice                    tensor.cuh:184-199
 *   rn_load_f32_file             <- Tensor::loadToCuda                  tensor.cuh:126-152
 *   rn_save_f32_file             <- Tensor::save                        tensor.cuh:154-163
 *   rn_sync                      <- cudaDeviceSynchronize + gpuAssert   nn.cu:14-15
 *
 * Not in the reference: rn_conv2d_grouped_* (torch's `groups`, ResNeXt's conv2) and rn_model_create_ex
 * (torchvision's ResNeXt / Wide ResNet networks on the same driver).
 *
 * The model entry points replace the reference driver
 * (cuda/inference/main.cu:53-226,243-251): createLayer/createResnet152,
 * layerForward/resnet152Forward and the host argmax.
 *
 * Layout.  The reference is NCHW everywhere.  With the context in
 * RN_LAYOUT_NCHW (default) every op reads and writes exactly what the
 * reference kernel does: 1x1 / padding-0 convolutions on an NCHW-native
 * contraction that takes the OIHW weight as it is, other convolutions through
 * a transpose of their input into context scratch, batch-norm and the
 * network's two pools on NCHW forms of their own.  The engine itself runs
 * NHWC: in RN_LAYOUT_NHWC the same entry points take [B,H,W,C] activations
 * (shape arguments unchanged), and rn_conv2d_nhwc_forward takes weights
 * pre-packed by rn_conv2d_pack_weight plus an optional fused epilogue.
 *
 * Aliasing: out == inp is allowed for relu, batchnorm2d and add (out may alias
 * inp1), as the reference driver uses them (main.cu:138,145-146,162-163).
 * conv, pool and linear must not alias.
 *
 * Alignment.  Callers hand these entry points slices of larger buffers (t.data() + offset).
 * The fp32 entry points -- the seven reference ops, rn_argmax_forward (logits; its idx: 8 bytes),
 * rn_nchw_to_nhwc, rn_nhwc_to_nchw, rn_nchw_to_nhwc_pad(_dt), rn_conv2d_pack_weight,
 * rn_batchnorm2d_fold, rn_conv2d_nhwc_forward with every operand of its epilogue -- accept any
 * 4-byte-aligned pointer for every operand and compute the same values; they are fastest with
 * every operand on a 16-byte boundary, where the float4 kernels and the matrix-core contraction
 * run.  Off it they take an element-wise kernel with the same bits (ReLU, add, batch-norm, pools,
 * layout changes) or, for rn_conv2d_forward, either the NCHW-native kernel (dword gathers and
 * stores; NCHW context, 1x1 / padding 0, or k x k with rn_ctx_set_nchw_taps) or the direct kernel
 * in the reference's summation order.  The contraction itself touches its operands in 16-byte
 * pieces, so rn_linear_forward (inp, out, weight, bias) and rn_conv2d_nhwc_forward (inp, out,
 * packed_weight, scale, shift, residual) run the direct kernel -- one thread per output, no matrix
 * cores, the price of a slice nobody has measured on network-sized layers -- as soon as ONE of
 * them is off a 16-byte boundary: a parameter arena that packs scale / shift vectors back to back
 * wants channel counts that are multiples of 4.  rn_nchw_to_nhwc_pad_dt(BF16) takes a dst on any
 * 2-byte boundary.  rn_nhwc_to_nchw_dt takes a dst on any 4-byte boundary in both element types and keeps
 * its 16-byte stores there (only its src decides between the fast and the element-wise form); so do the
 * stage maps of rn_model_forward_maps, which are its dst.
 * The grouped convolution (rn_conv2d_grouped_forward, rn_conv2d_grouped_nhwc_forward_dt in fp32) follows the
 * same rule: matrix cores with every operand on a 16-byte boundary, the direct kernel in the reference's
 * summation order otherwise; its bf16 form is rn_conv2d_nhwc_forward_dt(BF16) and refuses like it.
 * These must be 16-byte aligned and are refused with RN_ERR_INVALID (nothing is launched,
 * rn_last_error names the alignment) otherwise: every tensor, panel, scale / shift vector and
 * residual of rn_conv2d_nhwc_forward_dt(BF16), rn_conv2d_nhwc_pair_forward_dt,
 * rn_conv_chain_forward_dt, rn_conv_chain_pair_forward_dt; inp / out of
 * rn_maxpool2d_nhwc_forward_dt(BF16) and rn_avgpool2d_nhwc_forward_dt(BF16); inp / out /
 * packed_weight of rn_stem_pool_forward_dt and rn_stem_pool_nchw_forward_dt, and stem_out of
 * rn_stem_conv_pool_nchw_forward (their scale / shift are read element by element: 4 bytes); of
 * rn_conv2d_nhwc_exact_forward everything but inp_padded (dword gathers: 4 bytes).  The deferred
 * route (rn_ctx_set_deferred) folds a convolution with the ops behind it only when inp, out and
 * weight sit on 16-byte boundaries, the residual add only when its other operand does, and runs
 * what it does not fold literally.  tests/test_views_gpu.py holds each sentence of this paragraph
 * on views between guard bands.
 *
 * Threading: one context per host thread; a context = (device, stream,
 * scratch).  No global mutable state.  A host thread may own contexts on
 * several devices: every entry point makes its context's device the calling
 * thread's current HIP device before it touches the device.
 */
#ifndef RN_HIP_H
#define RN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RN_API __attribute__((visibility("default")))
#else
#define RN_API
#endif

typedef struct rn_ctx rn_ctx;
typedef struct rn_model rn_model;
typedef struct rn_event rn_event;

enum {
    RN_OK = 0,
    RN_ERR_INVALID = 1,     /* bad argument / shape precondition (reference: assert) */
    RN_ERR_HIP = 2,         /* HIP runtime error (reference: gpuAssert -> abort)      */
    RN_ERR_IO = 3,          /* file could not be opened / short read                  */
    RN_ERR_NOMEM = 4,
    RN_ERR_UNSUPPORTED = 5
};

enum { RN_LAYOUT_NCHW = 0, RN_LAYOUT_NHWC = 1 };

/* element types of the engine-side ("_dt") entry points; accumulation is always fp32 */
enum { RN_DTYPE_F32 = 0, RN_DTYPE_BF16 = 1 };

/* forward modes of rn_model_forward */
enum {
    RN_FWD_REFERENCE_OPS = 0, /* one kernel per reference op, same sequence as main.cu:168-226 */
    RN_FWD_FUSED = 1          /* BN / ReLU / residual add folded into the conv epilogue        */
};

/* ---- context ----------------------------------------------------------- */
RN_API int rn_ctx_create(rn_ctx **out, int device, void *hip_stream /* NULL: own stream */);
/* On a context with deferred state (rn_ctx_set_deferred, below) destroy runs what is recorded and gives
 * every caller buffer that the route holds as NHWC its NCHW content back, then waits for the stream.
 * So memory that was handed to a deferred context must still be allocated when the context is
 * destroyed: free it through that context first (rn_free takes the buffer out of the route's books), or
 * rn_observe it (it is NCHW then and destroy leaves it alone) -- a buffer freed behind the context's back
 * would be written after its free. */
RN_API int rn_ctx_destroy(rn_ctx *ctx);
RN_API int rn_ctx_set_layout(rn_ctx *ctx, int layout);
RN_API int rn_ctx_get_layout(const rn_ctx *ctx);
/* 1: synchronise and check after every op, like the reference (nn.cu:14-15). Default 0. */
RN_API int rn_ctx_set_sync_each_op(rn_ctx *ctx, int on);
/* Deferred execution of the reference's op-by-op call sequence (main.cu:127-166: conv.forward,
 * bn.forward in place, [addForward in place], reluForward in place -- separate launches, each a pass
 * over its tensor).  on = 1: with the context in its NCHW layout the seven reference entry points
 * (rn_conv2d_forward, rn_batchnorm2d_forward, rn_relu_forward, rn_add_forward, rn_maxpool2d_forward,
 * rn_avgpool2d_forward, rn_linear_forward) only RECORD their call and return.  The recorded list runs
 * when something is observed -- rn_memcpy_d2h / rn_save_f32_file, rn_sync, rn_flush, rn_observe,
 * rn_event_record, rn_free, a write into a buffer it names, or any other entry point -- and then a
 * convolution with the in-place batch-norm / add / ReLU that follow it on its output buffer is ONE
 * launch of the NHWC contraction with the fused epilogue (folded batch-norm, residual, ReLU), which
 * writes NHWC into the caller's own output buffer.  The context remembers which caller buffers hold
 * NHWC: ops that follow run on them as NHWC (no transposes between the first and the last op of a
 * network), and a buffer gets its NCHW content back only when it is observed (a whole-tensor
 * rn_memcpy_d2h transposes on its way out; rn_observe, partial reads, device-to-device copies and
 * entry points outside the seven rewrite the buffer in place first).  Every buffer named as an output
 * holds its value once the list has run: only in-place chains are folded, nothing is skipped.  Where
 * such a group is conv3 + bn + add + ReLU of a 64-channel bottleneck block and the next recorded group
 * is conv1 + bn + ReLU of the following block on that output, both run as one launch
 * (rn_conv_chain_forward_dt: the block output is written on its way to conv1; the same bits as the two
 * launches; RN_DEFER_CHAINS=0 in the environment keeps them apart).  The projection shortcut of a
 * stage's first block (a convolution of the same output with its in-place batch-norm, main.cu:131-137)
 * may stand between the two: it then runs right behind that launch, which nothing can observe as long as
 * neither group names a buffer the other writes (checked; otherwise the call order is kept).
 * Contract for the caller: device memory it handed to the seven ops is read and written by other
 * means (own kernels, hipMemcpy) only after rn_observe(ctx, ptr) -- the C++ veneer's Tensor::data()
 * does that.  rn_sync, rn_flush and rn_event_record RUN the list but leave the buffers NHWC (and
 * tagged): another stream or another context that reads such a buffer must see rn_observe(ctx, ptr)
 * first, however the two are ordered otherwise.  rn_ctx_destroy, rn_ctx_set_deferred(ctx, 0) and a
 * change of rn_ctx_set_layout give every buffer its NCHW content back.  Such memory is freed through
 * this context (rn_free) or observed first, and is still allocated when the context is destroyed (see
 * rn_ctx_destroy).  Weights and batch-norm parameters are cached in packed / folded form per buffer, by
 * pointer.  The caches follow writes made by: the seven recorded ops (an rn_add_forward or
 * rn_relu_forward whose output is a parameter buffer: the ops behind it in the list use the new
 * content, the ones in front of it the old); rn_memcpy_h2d, rn_memcpy_d2d and rn_memset; rn_free.
 * Switching the route off forgets them, so the seven ops may write parameters while they run
 * literally.  Any other writer -- an entry point outside the seven, the caller's own kernels, a
 * hipMemcpy -- is the caller's promise not to change a parameter buffer the route has seen (with
 * rn_ctx_set_weight_cache(ctx, 1) the packed panels are that cache's as well and keep its rule while
 * the route is off).
 * Numerics: the folded batch-norm is one fp32 fmaf per element instead of ops.cu:150's double
 * expression (<= 2e-5 on ResNet logits; the same epilogue as RN_FWD_FUSED).  on = 0 (default): every
 * call launches at once on NCHW tensors, the parity baseline; switching off runs what is recorded and
 * gives every buffer its NCHW content back. */
RN_API int rn_ctx_set_deferred(rn_ctx *ctx, int on);
RN_API int rn_ctx_get_deferred(const rn_ctx *ctx);
/* run the recorded ops now (asynchronously, on the context's stream) */
RN_API int rn_flush(rn_ctx *ctx);
/* run the recorded ops and make the caller buffer at dev_ptr hold its NCHW content */
RN_API int rn_observe(rn_ctx *ctx, const void *dev_ptr);
/* counters of the deferred route: ops recorded and not yet run, caller buffers currently NHWC, launches
 * with a folded chain, literal launches, layout passes (transposes) so far; any pointer may be NULL */
RN_API int rn_ctx_deferred_stats(const rn_ctx *ctx, uint64_t *pending_ops, uint64_t *nhwc_buffers,
                                 uint64_t *fused_launches, uint64_t *literal_launches,
                                 uint64_t *transposes);
/* Tile shape of the contraction kernel: 0 = chosen per launch (default), 1..N = force
 * candidate i (all candidates give bit-identical results; used by rn_model_tune). */
/* rn_conv2d_forward (the reference's OIHW / NCHW signature) re-packs the weight into the
 * engine's K-major panel on every call (not for 1x1 convolutions on NCHW tensors: their kernel
 * reads the OIHW buffer itself).  With the cache on, the panel is packed once per
 * (weight buffer, shape) and reused; entries die when the buffer is rn_free'd or written by
 * rn_memcpy_h2d / rn_memcpy_d2d / rn_memset.  A caller that turns it on promises not to change
 * a weight buffer by any other means (the reference's layers own their weights and never
 * do: nn.cuh:13,47-48,104).  Off by default; the C++ veneer turns it on. */
RN_API int rn_ctx_set_weight_cache(rn_ctx *ctx, int on);
/* kernel launches issued through this context so far (a contraction whose tail tiles are cut
 * into K chunks is two launches: the pieces and the kernel that adds them) */
RN_API uint64_t rn_ctx_launch_count(const rn_ctx *ctx);
RN_API int rn_conv_tile_candidates(void);
RN_API int rn_ctx_set_conv_tile(rn_ctx *ctx, int candidate);
/* Latency mode: max_splits > 1 lets a contraction whose output tiles cannot fill the chip
 * (small batches: B = 1 has 8 tiles of 64x64 in layer4's 3x3 convolutions, on 256 CUs) split
 * its K loop over up to max_splits blocks per tile; partial sums meet in context scratch and
 * a second kernel adds them in split order and applies the epilogue.  Deterministic, but the
 * summation order (and so the last bits) differs from the unsplit launch: 0 (default) keeps
 * results independent of the batch size.  Range 0..64. */
RN_API int rn_ctx_set_split_k(rn_ctx *ctx, int max_splits);
/* Fused stem + max-pool (rn_stem_pool_forward_dt): a block walks `items` consecutive items (four
 * stem rows = two pooled rows each) of one image; 0 (default) = chosen per launch so that the
 * blocks fill the device's CUs in the fewest rounds.  The bits do not depend on it: a block that
 * starts inside an image computes the one stem row above its segment once more. */
RN_API int rn_ctx_set_stem_items(rn_ctx *ctx, int items);
/* Tile order of the fp32 / bf16 4-wave contraction over the 8 XCDs (each with an L2 of its own): the tiles
 * are dealt as contiguous ranges of an order that keeps an XCD to one of `groups` groups of N tiles -- its
 * slice of the weight panel stays in that L2 while the M panels go by, the input is fetched by `groups`
 * XCDs.  0 (default): chosen per launch from the sizes of the input and of the weight panel; 1: M panel
 * major (an XCD reads its input rows once and streams the whole weight panel); 2 / 4 / 8: forced (also
 * RN_XCD_NGROUPS in the environment at context creation).  Changes which block computes a tile, no bit. */
RN_API int rn_ctx_set_xcd_groups(rn_ctx *ctx, int groups);
/* rn_conv2d_forward on NCHW tensors (RN_LAYOUT_NCHW, not deferred), kernel_size > 1: 0 = transpose the input into
 * scratch and run the NHWC contraction (its epilogue writes NCHW); 2 = gather the taps from the channel planes
 * (rn_conv_nchw.hip) wherever the shape is eligible (in_channels % 32 == 0, kernel_size <= 7); 1 (default) = gather
 * on planes of 2048 pixels or more, where it measures faster (tools/nchw_bench.py).  Also RN_NCHW_TAPS in the
 * environment at context creation.  Changes the route, no bit. */
RN_API int rn_ctx_set_nchw_taps(rn_ctx *ctx, int mode);
/* fp32 k x k convolutions with padding: pixel-major tiles.  An M tile of the contraction is then one output
 * pixel of a block of images instead of consecutive (b, oh, ow) rows, so the taps that fall into the padding are
 * the same for the whole tile and their K tiles are not multiplied at all (the row-major schedule multiplies
 * them as zeros).  No tensor changes its layout.  Eligible: fp32 in and out, kernel_size > 1, padding > 0,
 * in_channels % 32 == 0, dilation 1, one source, NHWC output, no split K, every output pixel with a tap inside
 * the image.  mode 0 (default): the library's rule (rn_conv_tap_skip_plan says what it decides); 1: never;
 * 2: wherever eligible.  Also RN_TAP_SKIP in the environment at context creation.  Only products with a zero
 * operand are left out: for finite operands the result is bit for bit that of mode 1; a non-finite weight
 * opposite padding (0 * Inf) no longer reaches the sum, as in the reference, which skips those taps too. */
RN_API int rn_ctx_set_tap_skip(rn_ctx *ctx, int mode);
/* Pixel-major launches issued through this context and the K tiles (128 bytes of K per tile row) they left out. */
RN_API int rn_ctx_tap_skip_stats(const rn_ctx *ctx, uint64_t *launches, uint64_t *k_tiles_skipped);
/* Pure host arithmetic, no device: the pixel-major plan of one convolution launch on tile candidate `tile`
 * (1..8 as rn_ctx_set_conv_tile; 0 = the tile the library chooses for the shape).  dtype is that of input and
 * output.  Returns 1 when the shape is eligible, 0 when not (the outputs are then 0), -1 for bad arguments.
 * m_tiles: h_out * w_out * ceil(B / BM); k_tiles: K tiles of the launch in the row-major count,
 * m_tiles * N tiles * (k * k * in_channels / 32); k_tiles_skipped: those a pixel-major launch leaves out;
 * rule: 1 when mode 0 takes the pixel-major tiles for this launch.  Any output may be NULL. */
RN_API int rn_conv_tap_skip_plan(int dtype, uint64_t B, uint64_t in_channels, uint64_t out_channels, uint64_t H,
                                 uint64_t W, uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                 uint64_t dilation, int tile, uint64_t *m_tiles, uint64_t *k_tiles,
                                 uint64_t *k_tiles_skipped, int *rule);
/* Diagnostics: device buffer of 16 x uint64 per block that the contraction kernel fills with
 * wall-clock and shader-clock stamps of its phases (tools/conv_stamps.py); NULL (default) = off. */
RN_API int rn_ctx_set_debug_stamps(rn_ctx *ctx, void *dev_buffer);
RN_API void *rn_ctx_stream(rn_ctx *ctx);
RN_API int rn_ctx_device(const rn_ctx *ctx);
RN_API int rn_sync(rn_ctx *ctx);
RN_API const char *rn_last_error(const rn_ctx *ctx);
RN_API const char *rn_status_string(int status);
RN_API int rn_device_count(int *count);
/* Where a device sits in the host: PCI address ("0000:c1:00.0"), the NUMA node of its slot and the
 * CPUs local to it as Linux lists them ("0-47,96-143"); -1 / "" where sysfs does not say.  The
 * host threads of rn_shard_* run on those cores. */
RN_API int rn_device_locality(int device, char *pci_bus_id, uint64_t pci_cap, int *numa_node,
                              char *cpulist, uint64_t cpulist_cap);
RN_API const char *rn_version(void);

/* ---- buffers ------------------------------------------------------------ */
RN_API int rn_malloc(rn_ctx *ctx, void **dev_ptr, uint64_t bytes);
RN_API int rn_free(rn_ctx *ctx, void *dev_ptr);
RN_API int rn_memcpy_h2d(rn_ctx *ctx, void *dev_dst, const void *host_src, uint64_t bytes);
RN_API int rn_memcpy_d2h(rn_ctx *ctx, void *host_dst, const void *dev_src, uint64_t bytes);
RN_API int rn_memcpy_d2d(rn_ctx *ctx, void *dev_dst, const void *dev_src, uint64_t bytes);
RN_API int rn_memset(rn_ctx *ctx, void *dev_ptr, int byte_value, uint64_t bytes);
/* whole file -> new device buffer; numel = file_size / 4 (tensor.cuh:138) */
RN_API int rn_load_f32_file(rn_ctx *ctx, const char *path, float **dev_ptr, uint64_t *numel);
RN_API int rn_save_f32_file(rn_ctx *ctx, const char *path, const float *dev_ptr, uint64_t numel);

/* ---- timing (HIP events on the context's stream) ------------------------ */
RN_API int rn_event_create(rn_ctx *ctx, rn_event **out);
RN_API int rn_event_destroy(rn_event *ev);
RN_API int rn_event_record(rn_ctx *ctx, rn_event *ev);
RN_API int rn_event_elapsed_ms(rn_event *start, rn_event *stop, float *ms); /* syncs on stop */

/* ---- the seven reference ops -------------------------------------------- */
RN_API uint64_t rn_conv_output_size(uint64_t x, uint64_t kernel_size, uint64_t stride,
                                    uint64_t padding);
RN_API int rn_conv2d_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight,
                             uint64_t kernel_size, uint64_t stride, uint64_t padding,
                             uint64_t h_out, uint64_t w_out, uint64_t B, uint64_t in_channels,
                             uint64_t out_channels, uint64_t H, uint64_t W);
RN_API int rn_maxpool2d_forward(rn_ctx *ctx, const float *inp, float *out, uint64_t kernel_size,
                                uint64_t stride, uint64_t padding, uint64_t h_out, uint64_t w_out,
                                uint64_t B, uint64_t channels, uint64_t H, uint64_t W);
RN_API int rn_avgpool2d_forward(rn_ctx *ctx, const float *inp, float *out, uint64_t kernel_size,
                                uint64_t stride, uint64_t padding, uint64_t h_out, uint64_t w_out,
                                uint64_t B, uint64_t channels, uint64_t H, uint64_t W);
RN_API int rn_linear_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight,
                             const float *bias /* nullable */, uint64_t B, uint64_t in_features,
                             uint64_t out_features);
RN_API int rn_relu_forward(rn_ctx *ctx, const float *inp, float *out, uint64_t N);
RN_API int rn_batchnorm2d_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight,
                                  const float *bias, const float *mean, const float *var,
                                  uint64_t B, uint64_t C, uint64_t N);
RN_API int rn_add_forward(rn_ctx *ctx, const float *inp1, const float *inp2, float *out,
                          uint64_t N);
/* host argmax of main.cu:243-251 as a device op: first maximum wins. idx is a device buffer. */
RN_API int rn_argmax_forward(rn_ctx *ctx, const float *logits, uint64_t *idx, uint64_t B,
                             uint64_t classes);

/* ---- the head behind the logits: softmax, top-k, both from one read (rn_head.hip) ----------------
 * fp32 rows [B, classes].  Float operands on any 4-byte boundary, uint64_t operands on an 8-byte boundary
 * (as rn_argmax_forward's idx); asynchronous on the context's stream, one launch each, counted by
 * rn_ctx_launch_count.  B == 0: RN_OK, nothing launched.  A null operand (probs of the fused call may be
 * NULL), an operand off its boundary, classes outside 1..65536 or k outside 1..min(classes, 64):
 * RN_ERR_INVALID, nothing launched, rn_last_error names the argument.
 *   Order.  (v_i, i) precedes (v_j, j) when v_i > v_j, or when v_i == v_j and i < j: a total order (-0.0 ==
 *     +0.0: the lower index first), so the result depends on neither B, the row's place in the batch, the
 *     alignment nor the launch.  Top-k is np.argsort(-x, kind="stable")[:k]; for finite rows k = 1 gives
 *     rn_argmax_forward's index.  A NaN ranks as -inf (argmax_kernel's rule; its value is returned as it
 *     is).  rn_argmax_forward's exception -- a NaN at index 0 is never displaced -- is taken for k = 1
 *     only: with k > 1 a NaN at index 0 ranks as -inf like any other.
 *   Probabilities.  p = expf(x - max) / sum, sum over expf(x - max) of the row: one max, one summation
 *     order (fixed by the kernel's block of 256 threads, nothing else) and one correctly rounded division
 *     in all three entry points, so rn_softmax_topk_forward's topk_prob[j] is bit for bit
 *     probs[topk_idx[j]] and what rn_softmax_forward writes there.  -inf entries (masked classes) give
 *     exactly 0; a row whose maximum is +inf and a row of -inf only give NaN, as torch does.
 *   The fused call ranks BY LOGIT, not by probability: exp is monotone but rounds, two distinct logits can
 *     share a probability; topk_idx is rn_topk_forward(logits)'s, bit for bit.
 *   One block per row; a row of up to 4096 classes is read from memory once (it lives in LDS), a longer
 *     one once per pass (maximum, sum, each top-k round, probabilities).  probs may alias logits. */
/* probs[b][c] = exp(x[b][c] - max_b) / sum_c exp(x[b][c] - max_b) */
RN_API int rn_softmax_forward(rn_ctx *ctx, const float *logits, float *probs, uint64_t B, uint64_t classes);
/* the k largest of each row, descending; equal values in ascending index order: values / indices [B, k] */
RN_API int rn_topk_forward(rn_ctx *ctx, const float *x, float *values, uint64_t *indices, uint64_t B,
                           uint64_t classes, uint64_t k);
/* one launch: probs (nullable, [B, classes]) and the k best classes ordered by logit with their probabilities */
RN_API int rn_softmax_topk_forward(rn_ctx *ctx, const float *logits, float *probs /* nullable */, float *topk_prob,
                                   uint64_t *topk_idx, uint64_t B, uint64_t classes, uint64_t k);

/* ---- layout converters and weight packing -------------------------------- */
RN_API int rn_nchw_to_nhwc(rn_ctx *ctx, const float *src, float *dst, uint64_t B, uint64_t C,
                           uint64_t H, uint64_t W);
RN_API int rn_nhwc_to_nchw(rn_ctx *ctx, const float *src, float *dst, uint64_t B, uint64_t C,
                           uint64_t H, uint64_t W);
/* NHWC [B,H,W,C] of `dtype` (RN_DTYPE_F32 or RN_DTYPE_BF16) -> NCHW [B,C,H,W] fp32; bf16 is widened exactly (its
 * bits shifted left by 16).  The form a model hands its stage maps out in (rn_model_forward_maps).  Any C, H, W
 * >= 1 (each, and H * W, below 2^31) and any B (more than 65535 images run as several launches); offsets are 64-bit
 * per image, so a dst of more than 2^31 bytes is legal.  dst_nchw on any 4-byte boundary, src_nhwc aligned to its
 * element (RN_ERR_INVALID otherwise, rn_last_error names the operand); asynchronous on the context's stream.
 * Fast form -- C % 4 == 0 (bf16: % 8) and src_nhwc on a 16-byte boundary, what a model's tensors always meet:
 * 16-byte loads along C, a padded LDS tile, 16-byte stores along H * W wherever four consecutive outputs share an
 * aligned 16 bytes of dst, whatever H * W and dst's address are (a 7 x 7 map: a block's 32 or 64 channels are one
 * contiguous span of dst with a scalar head and tail).  Any other shape: one element per thread, the same bits. */
RN_API int rn_nhwc_to_nchw_dt(rn_ctx *ctx, int dtype, const void *src_nhwc, float *dst_nchw, uint64_t B,
                              uint64_t C, uint64_t H, uint64_t W);
/* channels of the engine-side input image for a convolution: in_channels, or 4 when
 * in_channels < 4 (the 3-channel stem reads a [B,H,W,4] zero-padded image). */
RN_API uint64_t rn_conv2d_input_channels(uint64_t in_channels);
/* NCHW [B,C,H,W] -> NHWC with the channel dimension zero-padded to Cpad */
RN_API int rn_nchw_to_nhwc_pad(rn_ctx *ctx, const float *src, float *dst, uint64_t B, uint64_t C,
                               uint64_t H, uint64_t W, uint64_t Cpad);
RN_API uint64_t rn_conv2d_packed_weight_numel(uint64_t in_channels, uint64_t out_channels,
                                              uint64_t kernel_size);
/* OIHW (the weights_bin file order) -> K-major panel [Cout][kh][kw][Cin] the GEMM reads */
RN_API int rn_conv2d_pack_weight(rn_ctx *ctx, const float *weight_oihw, float *packed,
                                 uint64_t in_channels, uint64_t out_channels,
                                 uint64_t kernel_size);
/* scale = w / sqrt(var + 1e-5), shift = b - mean * scale, evaluated in double */
RN_API int rn_batchnorm2d_fold(rn_ctx *ctx, const float *weight, const float *bias,
                               const float *mean, const float *var, float *scale, float *shift,
                               uint64_t C);

typedef struct rn_epilogue {
    const float *scale;    /* per out-channel multiplier, NULL = 1 */
    const float *shift;    /* per out-channel addend,     NULL = 0 */
    const void *residual;  /* NHWC tensor of the output's shape and element type, added after
                              scale/shift; NULL = none */
    int relu;              /* apply max(x, 0) last */
} rn_epilogue;

/* NHWC in / NHWC out, packed weights, optional fused epilogue.  The input must have
 * rn_conv2d_input_channels(in_channels) floats per pixel. */
RN_API int rn_conv2d_nhwc_forward(rn_ctx *ctx, const float *inp, float *out,
                                  const float *packed_weight, uint64_t kernel_size,
                                  uint64_t stride, uint64_t padding, uint64_t h_out,
                                  uint64_t w_out, uint64_t B, uint64_t in_channels,
                                  uint64_t out_channels, uint64_t H, uint64_t W,
                                  const rn_epilogue *epilogue /* nullable */);

/* ---- element-type tagged engine entry points (bf16 storage, fp32 accumulate) ---------
 * The fp32 functions above are the dtype == RN_DTYPE_F32 case of these.  bf16 tensors
 * are NHWC only, 16-byte aligned, convolution in_channels a multiple of 64 (or the
 * small-Cin stem form, in_channels <= 4 and kernel_size <= 8, reading a 4-channel image that
 * carries its own zero border: padding = 0, even stride and width; its K tile is 8 pixels of
 * each of two consecutive image rows, so the 7x7 stem is 4 K tiles).                 */
RN_API uint64_t rn_conv2d_packed_weight_numel_dt(int dtype, uint64_t in_channels,
                                                 uint64_t out_channels, uint64_t kernel_size);
/* fp32 OIHW weights (the weights_bin order) -> K-major panel of `dtype` */
RN_API int rn_conv2d_pack_weight_dt(rn_ctx *ctx, int dtype, const float *weight_oihw, void *packed,
                                    uint64_t in_channels, uint64_t out_channels,
                                    uint64_t kernel_size);
/* fp32 NCHW [B,C,H,W] -> `dtype` NHWC [B, H+2*border, W+2*border, Cpad], zeros in the border
 * and in channels >= C */
RN_API int rn_nchw_to_nhwc_pad_dt(rn_ctx *ctx, int dtype, const float *src, void *dst, uint64_t B,
                                  uint64_t C, uint64_t H, uint64_t W, uint64_t Cpad,
                                  uint64_t border);
/* The same tensor from a decoder's output: 8-bit interleaved RGB [B,H,W,3] -> `dtype` NHWC
 * [B, H+2*border, W+2*border, Cpad] (Cpad 3 or 4), every element of it written by this launch,
 *     x = ((float)px / 255.0f - mean[c]) / std[c]
 * in fp32 with correctly rounded divisions: bit for bit what rn_nchw_to_nhwc_pad_dt(C = 3) writes
 * from the fp32 NCHW image that preprocess.py (the reference's) normalises on the host, for a
 * quarter of the bytes uploaded and no host arithmetic.  mean / std: three host floats each. */
RN_API int rn_image_u8_to_nhwc_pad_dt(rn_ctx *ctx, int dtype, const uint8_t *img, void *dst,
                                      uint64_t B, uint64_t H, uint64_t W, uint64_t Cpad,
                                      uint64_t border, const float mean[3], const float std[3]);
/* ---- resize and centre-crop of decoded images (the preset's first half, on the device) -------
 * What preprocess.preprocess_image_u8 does on the host with PIL -- short side to `resize` with the
 * antialiased bilinear reducer, centre crop of crop x crop -- byte for byte, for images of any size.
 * The arithmetic is PIL's 8-bit resample (preprocess.resize_crop_u8 restates it in numpy):
 *   geometry      W <= H: (nw, nh) = (resize, (int)((double)(resize * H) / W)), otherwise
 *                 (nw, nh) = ((int)((double)(resize * W) / H), resize);
 *                 left = round-half-even((nw - crop) / 2.0), top likewise;
 *   coefficients  per axis in -> out, in double: scale = in / out, fs = max(scale, 1), for output xx
 *                 center = (xx + 0.5) * scale, xmin = max((int)(center - fs + 0.5), 0),
 *                 xmax = min((int)(center + fs + 0.5), in) - xmin,
 *                 w[x] = max(0, 1 - |(x + xmin - center + 0.5) / fs|), divided by their sum (added in
 *                 index order), k[x] = (int)(0.5 + w[x] * 2^22); ksize = 2 * (int)ceil(fs) + 1;
 *   one pass      out = clip8((2^21 + sum px * k) >> 22) in int32;
 *   order         the horizontal pass first, rounded to 8 bits, the vertical pass on that result.
 * The coefficients are computed on the host (plain C doubles, no contraction into fma) and uploaded
 * with the batch; only the crop columns and crop rows that are read get any. */
RN_API int rn_resize_crop_geometry(uint64_t H, uint64_t W, uint64_t resize, uint64_t crop, uint64_t *nh,
                                   uint64_t *nw, uint64_t *top, uint64_t *left);
/* Pure host code: the table of outputs [first, first + count) of one axis.  bounds_out: count pairs
 * (xmin, xmax); coeffs_out: count rows of *ksize ints (the first xmax of a row are set, the rest 0);
 * cap: ints coeffs_out holds -- RN_ERR_INVALID when count * ksize > cap (ksize is still returned, so
 * a caller may ask with cap 0 first), or for a zero size or first + count > out_size. */
RN_API int rn_resize_coefficients(uint64_t in_size, uint64_t out_size, uint64_t first, uint64_t count,
                                  int32_t *bounds_out, int32_t *coeffs_out, uint64_t cap, uint64_t *ksize);
/* A ragged batch: packed_dev holds B interleaved 8-bit RGB images, image i at byte offsets[i] (any
 * offset: the loads assume no alignment) with heights[i] rows of widths[i] pixels; offsets, heights
 * and widths are host arrays.  dst: [B, crop, crop, 3] bytes on the device, any alignment.  One
 * launch (rn_resize.hip): a block owns a band of output rows of one image, runs the horizontal pass
 * of the source rows that band reads into LDS as bytes (64 KB of rows at a time, so any scale fits)
 * and the vertical pass out of LDS; nothing outside the crop is computed.  The call builds the
 * tables on the host, uploads them into context scratch and waits for that upload (the launch itself
 * is asynchronous), so it cannot be captured into a graph.
 * RN_ERR_INVALID, nothing launched, rn_ctx_launch_count unchanged: a null pointer (B > 0), an image
 * with a zero dimension, crop == 0, crop > resize, an image whose resized short or long side is
 * smaller than crop (the short side is `resize`, so never), or a dimension over the limits below.
 * B == 0 is RN_OK.  Limits: image sides <= 16384 (offsets and tap positions stay in 32 bits),
 * resize <= 16384, crop <= 2048 (a thread keeps 24 accumulators: one row of 3 * crop <= 256 * 24
 * bytes), scale = side / resized side <= 64 (the table of one image stays under 2 * crop * 133 ints;
 * a row of taps is at most 131 long). */
RN_API int rn_image_u8_resize_crop(rn_ctx *ctx, const uint8_t *packed_dev, const uint64_t *offsets,
                                   const uint64_t *heights, const uint64_t *widths, uint64_t B,
                                   uint8_t *dst_dev, uint64_t resize, uint64_t crop);
/* The two halves of that call, for callers that stage the table themselves (the host pipeline puts
 * it into its pinned staging behind the images): _table fills host memory (pure host code; with
 * table == NULL or cap too small it only returns the size in *bytes, and RN_ERR_INVALID for the
 * latter), _launch runs the kernel on a table that is already on the device, 16-byte aligned. */
RN_API int rn_image_u8_resize_crop_table(const uint64_t *offsets, const uint64_t *heights,
                                         const uint64_t *widths, uint64_t B, uint64_t resize, uint64_t crop,
                                         void *table, uint64_t cap, uint64_t *bytes);
RN_API int rn_image_u8_resize_crop_launch(rn_ctx *ctx, const uint8_t *packed_dev, const void *table_dev,
                                          uint64_t B, uint8_t *dst_dev, uint64_t crop);
/* inp/packed_weight of `dtype`, out and epilogue->residual of `out_dtype` */
RN_API int rn_conv2d_nhwc_forward_dt(rn_ctx *ctx, int dtype, int out_dtype, const void *inp,
                                     void *out, const void *packed_weight, uint64_t kernel_size,
                                     uint64_t stride, uint64_t padding, uint64_t h_out,
                                     uint64_t w_out, uint64_t B, uint64_t in_channels,
                                     uint64_t out_channels, uint64_t H, uint64_t W,
                                     const rn_epilogue *epilogue /* nullable */);
RN_API int rn_maxpool2d_nhwc_forward_dt(rn_ctx *ctx, int dtype, const void *inp, void *out,
                                        uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                        uint64_t h_out, uint64_t w_out, uint64_t B,
                                        uint64_t channels, uint64_t H, uint64_t W);
RN_API int rn_avgpool2d_nhwc_forward_dt(rn_ctx *ctx, int dtype, const void *inp, void *out,
                                        uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                        uint64_t h_out, uint64_t w_out, uint64_t B,
                                        uint64_t channels, uint64_t H, uint64_t W);
/* Global average over any H x W map: inp [B,H,W,channels] -> out [B,channels], both of `dtype` (what
 * torch's AdaptiveAvgPool2d(1) computes; the reference has no such op, its average pool takes one square
 * kernel_size).  The head of the model driver at every input size.  fp32 accumulator, sum / (H*W) in fp32,
 * rounded once to the storage type.  H == W == 7 runs the kernel of rn_avgpool2d_nhwc_forward_dt(k = 7) and
 * gives its bits.  Every other map: the taps of an output are split over up to 16 lanes and added in an
 * order that depends on (H, W) alone (written down above global_avgpool_kernel in rn_pool.hip), so an
 * image's result does not depend on B or on its place in the batch.
 * RN_ERR_INVALID, nothing launched: a null pointer, inp == out, channels % 4 != 0 (fp32) / % 8 != 0 (bf16),
 * inp or out off a 16-byte boundary, an unknown dtype.  B, channels, H or W == 0 is RN_OK. */
RN_API int rn_global_avgpool_nhwc_forward_dt(rn_ctx *ctx, int dtype, const void *inp, void *out, uint64_t B,
                                             uint64_t channels, uint64_t H, uint64_t W);

/* ---- grouped convolution (torch's `groups`): ResNeXt's conv2 ---------------------------------
 * weight [out_channels][in_channels / groups][k][k]; output channel o belongs to group
 * o / (out_channels / groups) and reads the input channels of that group only.  groups >= 2 and a
 * divisor of both channel counts (RN_ERR_INVALID otherwise; groups == 1 is rn_conv2d_forward /
 * rn_conv2d_nhwc_forward, whose kernels these entry points never reach), h_out / w_out must be the
 * convolution's output size.  Any kernel_size, stride and padding are computed.
 * Fast path (rn_conv_group.hip, v_mfma_f32_32x32x2_f32): fp32, kernel_size 3, in_channels ==
 * out_channels, a multiple of 32, Cg = in_channels / groups a divisor or a multiple of 32, every
 * operand (inp, out, weight, scale, shift, residual) on a 16-byte boundary.  The weight is packed
 * block-diagonally into super-groups of 32 output channels and the max(32, Cg) input channels they
 * read, zeros where a channel belongs to another group: 32 / Cg times the algorithmic products for
 * Cg < 32 (8x at Cg = 4), none wasted from Cg = 32 on.  Everything else -- other shapes, or ONE operand
 * off a 16-byte boundary (any 4-byte boundary is accepted) -- runs a direct kernel, one thread per
 * output in the reference's summation order (the ops.cu convolution loop over the group's channels,
 * bit for bit); both kernels read the same packed weight.  The summation order of an output element
 * depends on neither the batch size, the position in the batch nor the stream.
 * Non-finite inputs: on the fast path the structural zeros are multiplied like any weight, so a NaN
 * or an infinity in one group's input may surface in the other groups of its 32-channel super-group,
 * never outside it; the direct kernel keeps it inside its group.
 * bf16 storage (RN_DTYPE_BF16) has no grouped kernel of its own: pack_weight_dt expands the weight
 * to the dense [out][in][k][k] form with zeros outside the groups and packs the panel of the dense
 * bf16 contraction, forward_dt is rn_conv2d_nhwc_forward_dt on it (its conditions: in_channels % 64
 * == 0, 16-byte alignment).  Correct for every Cg, `groups` times the products, and a non-finite
 * input may surface in every output channel of the pixels that read it.
 * rn_conv2d_grouped_forward is the reference's conv2d signature plus `groups`: OIHW weight, tensors
 * in the context layout (NCHW: the input is transposed into scratch and the NHWC kernel writes
 * NCHW); the weight is packed into scratch per call.  On a deferred context (rn_ctx_set_deferred) it
 * runs what is recorded and then itself, at once: grouped convolutions are not recorded. */
RN_API int rn_conv2d_grouped_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight,
                                     uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                     uint64_t h_out, uint64_t w_out, uint64_t B, uint64_t in_channels,
                                     uint64_t out_channels, uint64_t H, uint64_t W, uint64_t groups);
RN_API uint64_t rn_conv2d_grouped_packed_weight_numel_dt(int dtype, uint64_t in_channels,
                                                         uint64_t out_channels, uint64_t kernel_size,
                                                         uint64_t groups);
RN_API int rn_conv2d_grouped_pack_weight_dt(rn_ctx *ctx, int dtype, const float *weight_oihw,
                                            void *packed, uint64_t in_channels, uint64_t out_channels,
                                            uint64_t kernel_size, uint64_t groups);
/* NHWC in / NHWC out, packed weight, optional fused epilogue; out and epilogue->residual of out_dtype */
RN_API int rn_conv2d_grouped_nhwc_forward_dt(rn_ctx *ctx, int dtype, int out_dtype, const void *inp,
                                             void *out, const void *packed_weight, uint64_t kernel_size,
                                             uint64_t stride, uint64_t padding, uint64_t h_out,
                                             uint64_t w_out, uint64_t B, uint64_t in_channels,
                                             uint64_t out_channels, uint64_t H, uint64_t W,
                                             uint64_t groups, const rn_epilogue *epilogue /* nullable */);

/* ---- dilated convolution (torch's `dilation`, one factor for rows and columns) -----------------
 * Kernel tap (kh, kw) of output (oh, ow) reads input (oh * stride - padding + kh * dilation,
 * ow * stride - padding + kw * dilation); a tap outside the image contributes nothing.  The weight,
 * its packed panels (rn_conv2d_pack_weight_dt for groups == 1, rn_conv2d_grouped_pack_weight_dt for
 * groups >= 2: dilation does not change a panel), the FLOPs and the summation order of an output
 * element are those of the undilated convolution of the same shape.
 * rn_conv_output_size_dilated = (x + 2 * padding - dilation * (kernel_size - 1) - 1) / stride + 1, and 0
 * where the dilated kernel does not fit the padded extent (or an argument that must be >= 1 is 0).
 * rn_conv2d_dilated_forward is the reference's conv2d signature plus `dilation` and `groups`: OIHW
 * weight, tensors in the context layout (NCHW: transposed into scratch, the contraction writes
 * NCHW); on a deferred context it runs what is recorded and then itself, at once.
 * rn_conv2d_dilated_nhwc_forward_dt is NHWC in / NHWC out with a packed weight and the fused epilogue.
 * With dilation == 1 (and for kernel_size == 1, whose one tap no dilation moves) both issue exactly the
 * launch of rn_conv2d_forward / rn_conv2d_grouped_forward and rn_conv2d_nhwc_forward_dt /
 * rn_conv2d_grouped_nhwc_forward_dt: the same bits.
 * Which kernel runs, dilation >= 2:
 *  - matrix cores, groups == 1: in_channels % 32 == 0 (fp32) or % 64 == 0 (bf16, required), kernel_size
 *    <= 15, tensors below 2^29 elements, every operand on a 16-byte boundary -- all tile candidates,
 *    the resident grids, split K, the chunked K sum and the bf16 256-wide tiles, each bit-identical
 *    to the others wherever the undilated layer's are;
 *  - matrix cores, groups >= 2: the fp32 super-group kernel under its undilated conditions (kernel_size
 *    3, in_channels == out_channels, ...); bf16 runs the dense contraction on the dense panel;
 *  - everything else in fp32 -- in particular the small-Cin (stem) packing, which has no dilated
 *    form, and an operand off a 16-byte boundary -- runs the direct kernel, one thread per output in
 *    the reference's summation order; the bf16 small-Cin form is RN_ERR_UNSUPPORTED;
 *  - never: the strip kernel, the exact-K packing, the NCHW-native kernel, the chained launches.
 * Alignment rules and non-finite behaviour are those of the undilated entry point of the same form
 * (a padded or never-reached tap is skipped, not multiplied by zero; the grouped fast path and the
 * bf16 grouped panel multiply their structural zeros, see above).
 * RN_ERR_INVALID, nothing launched: dilation == 0 or above RN_CONV_MAX_DILATION, h_out / w_out other
 * than rn_conv_output_size_dilated of H / W, groups that do not divide both channel counts. */
#define RN_CONV_MAX_DILATION 1024
RN_API uint64_t rn_conv_output_size_dilated(uint64_t x, uint64_t kernel_size, uint64_t stride,
                                            uint64_t padding, uint64_t dilation);
RN_API int rn_conv2d_dilated_forward(rn_ctx *ctx, const float *inp, float *out, const float *weight,
                                     uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                     uint64_t dilation, uint64_t h_out, uint64_t w_out, uint64_t B,
                                     uint64_t in_channels, uint64_t out_channels, uint64_t H, uint64_t W,
                                     uint64_t groups);
RN_API int rn_conv2d_dilated_nhwc_forward_dt(rn_ctx *ctx, int dtype, int out_dtype, const void *inp,
                                             void *out, const void *packed_weight, uint64_t kernel_size,
                                             uint64_t stride, uint64_t padding, uint64_t dilation,
                                             uint64_t h_out, uint64_t w_out, uint64_t B,
                                             uint64_t in_channels, uint64_t out_channels, uint64_t H,
                                             uint64_t W, uint64_t groups,
                                             const rn_epilogue *epilogue /* nullable */);

/* ---- model (main.cu driver) ---------------------------------------------- */
/* arch: 50, 101 or 152 (bottleneck blocks, counts 3/4/6/3, 3/4/23/3, 3/8/36/3), or 18 or 34
 * (torchvision's basic blocks -- two 3x3 convolutions, expansion 1, final width 512 -- counts
 * 2/2/2/2 and 3/4/6/3; tensor keys layerX.Y.{conv1,bn1,conv2,bn2,downsample.0,downsample.1}.*).
 * Fused basic blocks: conv1 + bn1 + ReLU, conv2 + bn2 + shortcut + ReLU; with pair fusion, block 0
 * of stages 2-4 runs conv2 and the downsample as one contraction (not bit-neutral, like the
 * bottleneck pair).  No chained launches in basic-block networks. */
RN_API int rn_model_create(rn_ctx *ctx, rn_model **out, int arch);
/* torchvision's bottleneck family by its constructor arguments: depth 50, 101 or 152 and
 * (groups, width_per_group) = (1, 64) ResNet -- the same model as rn_model_create(depth) --, (32, 4),
 * (32, 8), (64, 4) ResNeXt (resnext50_32x4d, resnext101_32x8d, resnext101_64x4d) or (1, 128) Wide ResNet
 * (wide_resnet50_2, wide_resnet101_2); anything else RN_ERR_UNSUPPORTED.  The bottleneck's middle
 * width is planes * width_per_group / 64 * groups; conv2 is a 3x3 convolution with `groups` groups
 * (rn_conv2d_grouped_nhwc_forward_dt), weight [width][width / groups][3][3]; tensor keys, stem, pools
 * and classifier are ResNet's.  Chained launches need (mid, channels) = (64, 256) / (128, 512) blocks:
 * these networks have none and run conv3 and conv1 as separate launches.  The tuning table's header
 * carries (groups, width_per_group): a table is refused by a model of another family. */
RN_API int rn_model_create_ex(rn_ctx *ctx, rn_model **out, int depth, int groups, int width_per_group);
RN_API int rn_model_destroy(rn_model *m);
/* Rows of the classifier: 1..65536, default 1000 (a fine-tuned checkpoint has fc.weight [classes, features]).
 * Legal until the first rn_model_set_tensor, rn_model_load_dir or rn_model_finalize; after any of those, and
 * for a count out of range, RN_ERR_INVALID and nothing changes.  It re-sizes the fc.weight / fc.bias entries
 * of the layer table (rn_model_tensor_key reports the new numel); the packed classifier panel, the logits
 * strides of every forward entry point (rn_model_forward, _u8, _images_u8, _outputs, rn_model_tune,
 * rn_model_capture, rn_pipeline_*) and the profile record follow it.  Tuning tables do not carry it: the
 * classifier launch is not in them, and every tile candidate is valid for any out_channels.
 * A count that is no multiple of 4 puts the logits rows of later sub-batches or parts off a 16-byte
 * boundary, where the contraction cannot write them.  fp32 models then run the classifier of EVERY launch
 * on the direct kernel (one thread per logit, the reference's summation order): correct, slow, and an
 * image's logits stay independent of the part it runs in.  bf16 models refuse such a count at
 * rn_model_finalize (RN_ERR_UNSUPPORTED).  rn_shard_* creates its own models and stays at 1000. */
RN_API int rn_model_set_classes(rn_model *m, uint64_t classes);
RN_API uint64_t rn_model_classes(const rn_model *m);
RN_API uint64_t rn_model_features(const rn_model *m); /* 512 (ResNet-18/34) or 2048 */
/* state_dict key -> host data; numel must match the layer table. */
RN_API int rn_model_set_tensor(rn_model *m, const char *key, const float *host_data,
                               uint64_t numel);
/* read every tensor from dir/<key> (the reference's weights_bin/ directory) */
RN_API int rn_model_load_dir(rn_model *m, const char *weights_dir);
/* storage type of activations and packed weights inside the model: RN_DTYPE_F32 (default)
 * or RN_DTYPE_BF16 (fused mode only).  Input images and logits stay fp32.  Call before
 * rn_model_finalize. */
RN_API int rn_model_set_dtype(rn_model *m, int dtype);
/* upload-side work done once: pack conv weights, fold batch-norms */
RN_API int rn_model_finalize(rn_model *m);
/* names of the tensors the loader expects, one per call; returns NULL past the end */
RN_API const char *rn_model_tensor_key(const rn_model *m, uint64_t index, uint64_t *numel);
/* The size of the images every forward entry point of this model reads: [B,3,H,W] floats or [B,H,W,3]
 * bytes (rn_model_forward, _u8, _outputs, _outputs_u8, rn_model_tune, rn_model_capture, rn_pipeline_create /
 * _u8).  Default 224 x 224; 32..2048 for each of H and W.  A property of the model, like the class count:
 * there is no per-call size.  Legal before or after rn_model_finalize (the weights do not depend on it).
 * RN_ERR_INVALID, nothing changed: a side out of range, a size of which not one image fits the kernels'
 * tensor range (none within 2048 x 2048), or a captured graph or a pipeline of this model alive (they hold
 * buffers of the old size).  It waits for the model's queued forwards, frees the activation arenas (the
 * next forward sizes them anew; rn_model_activation_bytes follows) and drops the tuned tiles.
 * What follows from the size:
 *   - the head pools whatever map the last stage leaves (H/32 x W/32, rounded up) with
 *     rn_global_avgpool_nhwc_forward_dt; at 224 x 224 that is the 7 x 7 launch and every bit of before;
 *   - the stem route.  The fused stem + max-pool launch (rn_stem_pool_forward_dt) is used where its
 *     conditions hold: conv output width a multiple of 8 and at most 128 (W a multiple of 16 up to 256, or
 *     one less), its LDS budget, bf16: an even W; the NCHW-fetching form (fusion 2) also W % 4 == 0.
 *     Otherwise stem and max-pool run as separate launches, as with rn_model_set_stem_pool_fusion(m, 0).
 *     The route depends on (H, W, dtype, settings) only, never on B: an image's logits stay independent of
 *     batch, part and sub-batch, bit for bit;
 *   - rn_model_max_sub_batch: the largest power of two, at most 512, for which the largest tensor of the
 *     arenas (per image: the padded input, the stem output, the first stage's output) times it stays below
 *     the kernels' 2^29 elements: 512 at 224 x 224, 16 at 1024 x 1024;
 *   - the tuning table's header carries the size in a word of its own that is absent for 224 x 224, whose
 *     tables keep their format; a model refuses a table measured at another size;
 *   - rn_model_forward_images_u8 and rn_pipeline_create_images_u8 stay at 224 x 224 (their contract is
 *     "resize 256, crop 224"): RN_ERR_UNSUPPORTED with rn_last_error's text on a model of another size.
 *     rn_shard_* creates its own models and stays at 224 x 224. */
RN_API int rn_model_set_input_size(rn_model *m, uint64_t H, uint64_t W);
RN_API int rn_model_input_size(const rn_model *m, uint64_t *H, uint64_t *W); /* either pointer may be NULL */
RN_API uint64_t rn_model_max_sub_batch(const rn_model *m);
/* torchvision's replace_stride_with_dilation (flags 0 or 1 for layer2, layer3, layer4): a flagged stage keeps
 * its input's resolution and dilates its 3x3 convolutions instead, so the backbone's output stride becomes 16, 8
 * or 4 (rn_model_output_stride; 32 undilated) -- the form DeepLab / FCN run these weights in.  The rule is
 * torchvision's _make_layer: a running dilation starts at 1; for a flagged stage previous = dilation,
 * dilation *= 2, stride = 1.  Block 0 of a stage runs conv2 at the stage's stride with dilation = padding =
 * previous and keeps its downsample 1x1 (at the stage's stride: the widths differ); blocks 1.. run conv2 with
 * dilation = padding = dilation; an unflagged stage uses the current dilation for all its blocks and keeps its
 * stride.  ResNet-50 with (0,1,1): layer3.0 d1, layer3.1-5 d2, layer4.0 d2, layer4.1-2 d4, final map 28 x 28 at
 * 224 x 224; with (1,1,1) the largest dilation is 8.  The dilated convolutions are
 * rn_conv2d_dilated_nhwc_forward_dt on the panels of the undilated model.
 * A property of the model, like the input size: legal before or after rn_model_finalize (the weights do not
 * depend on it).  RN_ERR_INVALID, nothing changed: a flag other than 0 or 1, flags of which not one image fits
 * the kernels' tensor range, or a captured graph or a pipeline of this model alive.  RN_ERR_UNSUPPORTED with
 * rn_last_error's text: ResNet-18/34 (torchvision raises NotImplementedError for BasicBlock).  It waits for the
 * model's queued forwards, frees the activation arenas and drops the tuned tiles.
 * What follows from the flags, as from the size: the arenas (each the maximum over all stages: layer4's output
 * of a (0,1,1) model at 224 x 224 is 28 * 28 * 2048 elements per image, twice the stem's; those of a (0,0,0)
 * model are what they were), rn_model_max_sub_batch (256 there) and rn_model_activation_bytes; the map the head
 * pools; the profile's FLOPs; block 0 of a dilated stage as a fused pair is the two-source launch with
 * stride2 == 1; every forward entry point, rn_model_tune, rn_model_capture and the pipelines
 * (rn_model_forward_images_u8 included: its contract is the 224 crop only).  The tuning table's header carries
 * the flags in a word of its own that is absent for (0,0,0), whose tables keep their format; a model refuses a
 * table measured under other flags.  rn_shard_* creates its own models and stays undilated. */
RN_API int rn_model_set_dilation(rn_model *m, int layer2, int layer3, int layer4);
RN_API int rn_model_dilation(const rn_model *m, int out[3]);
RN_API int rn_model_output_stride(const rn_model *m); /* 32, 16, 8 or 4 */
/* input: device NCHW [B,3,H,W] of the model's input size; logits: device [B,classes]. Asynchronous on the stream.
 *
 * Geometry of the model driver (the reference's -- main.cu:230 hard-codes {1, 3, 224, 224} -- is fixed):
 *   - images are 3 x H x W fp32, NCHW, H x W = rn_model_input_size (default 224 x 224).  The call has no size
 *     argument: a buffer of another geometry cannot be told apart, so callers that read files check the
 *     element count first (rn_infer does: --size H,W, and it refuses anything but B*3*H*W floats);
 *   - bottleneck depths 50 / 101 / 152, basic-block depths 18 / 34; the class count is not fixed either
 *     (rn_model_set_classes, default 1000);
 *   - any B >= 1: the kernels address a tensor with 32-bit byte offsets (2^29 fp32 elements; at 224 x 224
 *     the stem output of 669 images is the first to pass it), so a batch runs as sub-batches of at most
 *     rn_model_max_sub_batch images (512 at 224 x 224) through the same arenas, each as `streams` parts
 *     (rn_model_set_streams); every image's logits are independent of that split, bit for bit;
 *   - arenas: at 224 x 224 13.6 MB (fp32) / 6.8 MB (bf16) of activations per image of the largest
 *     sub-batch seen (basic-block networks: 8.5 / 4.2 MB), in proportion to H x W otherwise, allocated on
 *     first use (RN_ERR_NOMEM when the device cannot hold them). */
RN_API int rn_model_forward(rn_model *m, const float *input_nchw, uint64_t B, float *logits,
                            int mode);
/* The same forward from 8-bit RGB crops, [B,H,W,3] of the model's input size on the device: the first launch
 * (rn_image_u8_to_nhwc_pad_dt with the ImageNet mean (0.485, 0.456, 0.406) and std (0.229, 0.224,
 * 0.225)) replaces the layout launch of the float route and writes the same first tensor, so the
 * logits are those of rn_model_forward on the host-normalised image, bit for bit, for every
 * architecture, dtype, mode and batch split.  With rn_model_set_stem_pool_fusion(m, 2) -- patches
 * fetched from the caller's NCHW image -- there is no NCHW image to fetch from: the byte route
 * runs the padded-image form of the fused stem, as with fusion 1.  Tuned tiles (rn_model_tune, on
 * the float entry point) serve both routes. */
RN_API int rn_model_forward_u8(rn_model *m, const uint8_t *input_nhwc, uint64_t B, float *logits,
                               int mode);
/* The same forward from decoded images of any size: rn_image_u8_resize_crop(resize 256, crop 224) into
 * a buffer the model owns ([B,224,224,3] of the largest sub-batch seen), then exactly the launches of
 * rn_model_forward_u8 on it -- the logits are those of rn_model_forward_u8 on the crops PIL makes on
 * the host, bit for bit.  Same sub-batches (<= 512), streams and profiling (the launch is the op
 * "image_u8_resize_crop" of layer "input", the first record of a profiled forward) as the byte
 * route; the resize of a sub-batch runs on the model's own stream before the parts fork.  The
 * coefficient tables come from host memory that the call frees, so a stream that is being captured
 * is refused with RN_ERR_UNSUPPORTED.  Refusals of rn_image_u8_resize_crop apply (checked for the
 * whole batch before anything is launched).  A model whose input size is not 224 x 224:
 * RN_ERR_UNSUPPORTED. */
RN_API int rn_model_forward_images_u8(rn_model *m, const uint8_t *packed_dev, const uint64_t *offsets,
                                      const uint64_t *heights, const uint64_t *widths, uint64_t B,
                                      float *logits, int mode);
/* More than the logits from one forward.  Device pointers; any may be NULL; zero-initialise the struct. */
typedef struct rn_model_outputs {
    float *logits;       /* [B, classes]: bit for bit what rn_model_forward writes */
    float *features;     /* [B, features] fp32: the pooled values the classifier reads */
    float *probs;        /* [B, classes]: rn_softmax_forward of the logits */
    float *topk_prob;    /* [B, k] */
    uint64_t *topk_idx;  /* [B, k]: ordered by logit (rn_softmax_topk_forward) */
    uint64_t k;          /* 0 = no top-k; otherwise 1..min(classes, 64) with both topk pointers set */
} rn_model_outputs;
/* Exactly the launches of rn_model_forward / rn_model_forward_u8 -- same sub-batches (<= rn_model_max_sub_batch images), streams
 * and profile records -- and behind each sub-batch, on the model's own stream: the features (fp32 models: a
 * device-to-device copy out of the pooled arena; bf16 models: the bf16 values widened to fp32, exact; op
 * "features" of layer "head"), then at most one rn_softmax_topk_forward (op "softmax_topk"), or
 * rn_softmax_forward when k == 0 (op "softmax").  With logits == NULL the logits of a sub-batch go to a
 * buffer the model owns ([min(B, 512), classes] of the largest call seen, grown on first use like the
 * arenas: RN_ERR_INVALID while a captured graph of the context lives, RN_ERR_UNSUPPORTED on a stream that
 * is being captured).  Nothing to write (every pointer NULL and k == 0), or k > 0 without both topk
 * pointers or out of range: RN_ERR_INVALID.  Both forward modes. */
RN_API int rn_model_forward_outputs(rn_model *m, const float *input_nchw, uint64_t B,
                                    const rn_model_outputs *outs, int mode);
RN_API int rn_model_forward_outputs_u8(rn_model *m, const uint8_t *input_nhwc, uint64_t B,
                                       const rn_model_outputs *outs, int mode);
/* The feature maps behind layer1..layer4 from one forward, each [B, C, H, W] fp32 in the caller's device buffer
 * (torchvision's IntermediateLayerGetter; the backbone form DeepLab / FCN / FPN read).  NULL = not wanted. */
typedef struct rn_model_maps { float *layer[4]; } rn_model_maps;   /* layer1..layer4; NULL = not wanted */
/* C, H, W of the map behind stage 1..4 for the model's architecture, input size and dilation flags (ResNet-50 at
 * 224 x 224: 256 x 56 x 56 .. 2048 x 7 x 7; with (0,1,1) layer3 and layer4 at 28 x 28; ResNet-18: 64 .. 512
 * channels).  Legal before rn_model_finalize; any of the pointers may be NULL; stage outside 1..4: RN_ERR_INVALID. */
RN_API int rn_model_stage_shape(const rn_model *m, int stage /* 1..4 */, uint64_t *C, uint64_t *H, uint64_t *W);
/* Exactly the launches of rn_model_forward_outputs -- same sub-batches, parts, front slices and profile records,
 * the same bits in every head output -- plus one rn_nhwc_to_nchw_dt per wanted stage and launch batch (op
 * "stage_map", layer "layer1".."layer4" in the profile; bf16 models: the stored values widened exactly).  The
 * export is queued right behind the last block of its stage on the stream that block ran on, where the stage's
 * output still sits in its ping-pong arena (two blocks later it is overwritten); the parts' streams are joined
 * before the call's work on the model's stream ends, as for the logits.  outs may be NULL (or name nothing): the
 * logits then go to the buffer the model owns, as with outs->logits == NULL.  Both forward modes, every
 * architecture, input size and dilation.  No new arenas: rn_model_activation_bytes, rn_model_max_sub_batch and the
 * tuning table are what they were.  The request lives for this call only: no later forward, tune, capture or
 * pipeline submit exports anything.
 * Refused, nothing launched, nothing changed: maps == NULL, or all four stages NULL and nothing wanted in outs
 * (RN_ERR_INVALID, "nothing to write"); a stage pointer off a 4-byte boundary (RN_ERR_INVALID, rn_last_error names
 * the stage); a model that is not finalized, a bad mode, a bad top-k request (RN_ERR_INVALID); a bf16 model with
 * RN_FWD_REFERENCE_OPS (RN_ERR_UNSUPPORTED).  rn_model_capture, the pipelines and rn_shard_* carry no maps, and a
 * backbone-only forward still runs the head. */
RN_API int rn_model_forward_maps(rn_model *m, const float *input_nchw, uint64_t B, const rn_model_outputs *outs,
                                 const rn_model_maps *maps, int mode);
RN_API int rn_model_forward_maps_u8(rn_model *m, const uint8_t *input_nhwc, uint64_t B, const rn_model_outputs *outs,
                                    const rn_model_maps *maps, int mode);
/* ---- semantic segmentation: per-pixel scores upsampled to the image, and the label map ----------------------
 * Bilinear upsample of NHWC class scores [B, h, w, src_channels] fp32 to H x W, as NCHW scores [B, classes, H, W]
 * and / or as the label map [B, H, W] (one byte per pixel: the argmax over the classes), in ONE launch.  With
 * scores_nchw == NULL no score is written anywhere: the running maximum lives in registers and the launch moves
 * one byte per output pixel instead of 4 * classes.  Only channels 0 .. classes-1 of a source pixel are read;
 * src_channels >= classes is the pixel's pitch (the padded channel count a 1x1 convolution wrote).
 * The arithmetic is torch.nn.functional.interpolate(mode="bilinear", align_corners=False) with every operation
 * rounded to fp32 on its own, no product fused into an add.  Per axis n_in -> n_out, output index o:
 *     scale = (float)n_in / (float)n_out                       (one fp32 division, on the host)
 *     src   = max(fl(fl(scale * fl((float)o + 0.5f)) - 0.5f), 0.0f)
 *     i0    = min((int)src, n_in - 1);  i1 = min(i0 + 1, n_in - 1)
 *     l1    = fl(src - (float)i0);      l0 = fl(1.0f - l1)
 * and with row weights (a0, a1), column weights (b0, b1):
 *     top = fl(fl(b0 * v[y0][x0]) + fl(b1 * v[y0][x1]));  bot = the same on row y1
 *     out = fl(fl(a0 * top) + fl(a1 * bot))
 * (segmentation.upsample_bilinear_ref restates it in numpy; the kernel matches it bit for bit).  The label is the
 * lowest channel index that holds the maximum: channel 0 to start with, replaced only where v > best, which is
 * numpy.argmax on finite data.  A NaN score never replaces the best (and a NaN in channel 0 is never replaced).
 * Any ratio: enlarging is the purpose, H == h && W == w (the source's bits) and shrinking are correct as well.
 * classes 1..256 (a label fits a byte), src_channels <= 256 and a multiple of 4, h, w, H, W >= 1, h * w and H * W
 * below 2^31; offsets are 64-bit per image.  src_nhwc on a 16-byte boundary, scores_nchw on any 4-byte boundary,
 * labels anywhere: 16-byte score stores and 4-byte label stores are used wherever four consecutive outputs share
 * an aligned unit of the destination, whatever W and the addresses are.  Asynchronous on the context's stream;
 * allocates and uploads nothing, every parameter is a kernel argument (capturable).  B == 0: RN_OK, nothing
 * launched.  RN_ERR_INVALID, nothing launched, rn_last_error names the operand: ctx or src_nhwc NULL, both outputs
 * NULL, classes outside 1..256, src_channels < classes or no multiple of 4, a zero size, a misaligned src_nhwc or
 * scores_nchw. */
RN_API int rn_upsample_bilinear_forward(rn_ctx *ctx, const float *src_nhwc, uint64_t B, uint64_t h, uint64_t w,
                                        uint64_t classes, uint64_t src_channels, uint64_t H, uint64_t W,
                                        float *scores_nchw /* [B,classes,H,W] or NULL */,
                                        uint8_t *labels /* [B,H,W] or NULL */);
/* torchvision's FCNHead on any NHWC map, no model needed: Conv3x3(in, mid, padding 1, no bias) + BatchNorm + ReLU
 * (+ Dropout, the identity at inference) + Conv1x1(mid, classes) with bias, then the upsample above.  No convolution
 * code of its own: rn_batchnorm2d_fold, rn_conv2d_pack_weight_dt and two rn_conv2d_nhwc_forward_dt launches (the
 * 3x3 with the folded scale / shift and ReLU in its epilogue; the 1x1 with shift = bias and fp32 output whatever
 * the storage type, its out_channels rounded up to a multiple of 4 with zero rows so that every coarse pixel
 * starts on a 16-byte boundary: the src_channels of the upsample).  in_channels is a multiple of 64, classes
 * 1..256; mid_channels is a multiple of 64 where it comes from a backbone (layer4 of a bottleneck network: 2048 ->
 * 512; of a basic-block network: 512 -> 128) and may be any count 1..8192: the head rounds it up to a multiple of 64
 * inside (the bf16 contraction's K granule) with channels of zero weights, scale 0 and shift 0, which hold
 * ReLU(0) = 0 and add exact zeros to the 1x1 convolution's sums (FCNHead(128, 21) runs 128 -> 32 as 128 -> 64).
 * Tensors (rn_seg_head_set_tensor, fp32 host data, torchvision's keys and shapes): classifier.0.weight
 * [mid,in,3,3]; classifier.1.weight / .bias / .running_mean / .running_var [mid]; classifier.4.weight
 * [classes,mid,1,1]; classifier.4.bias [classes].  rn_seg_head_set_dtype (before finalize) chooses the storage
 * type of the input map, the mid tensor and the weight panels.  rn_seg_head_finalize folds and packs; it needs
 * every tensor.
 * rn_seg_head_forward: x_nhwc [B,h,w,in_channels] of the storage type (16-byte aligned) -> scores_nchw
 * [B,classes,H,W] and / or labels [B,H,W] (either may be NULL, not both): three launches on the context's stream.
 * The head owns its two scratch tensors (the mid tensor [B,h,w,mid] and the coarse scores [B,h,w,classes padded]
 * fp32); they grow on first use like the logits buffer a model owns: RN_ERR_UNSUPPORTED on a stream that is being
 * captured, RN_ERR_INVALID while a captured graph of the context lives. */
typedef struct rn_seg_head rn_seg_head;
RN_API int rn_seg_head_create(rn_ctx *ctx, rn_seg_head **out, uint64_t in_channels, uint64_t mid_channels,
                              uint64_t classes);
RN_API int rn_seg_head_set_dtype(rn_seg_head *hd, int dtype);
RN_API int rn_seg_head_set_tensor(rn_seg_head *hd, const char *key, const float *host_data, uint64_t numel);
RN_API int rn_seg_head_finalize(rn_seg_head *hd);
RN_API int rn_seg_head_destroy(rn_seg_head *hd);
RN_API int rn_seg_head_forward(rn_seg_head *hd, const void *x_nhwc, uint64_t B, uint64_t h, uint64_t w, uint64_t H,
                               uint64_t W, float *scores_nchw, uint8_t *labels);
/* Channel concat with a per-image broadcast source, ONE launch: dst [B, pixels, sum(channels) + per_image_channels]
 * = the n_src (1..8) sources srcs[i] [B, pixels, channels[i]] in order, then per_image [B, per_image_channels]
 * repeated at every pixel of its image (NULL with per_image_channels == 0: no broadcast).  All of `dtype` (fp32 or
 * bf16).  A copy in 16-byte units: bit for bit numpy.concatenate, NaN payloads and signed zeros included.  Every
 * channel count times the element size is a multiple of 16 bytes and every pointer 16-byte aligned, so every source
 * starts on a 16-byte boundary inside a destination pixel.  B * pixels below 2^31; offsets are 64-bit (B * pixels *
 * channels may pass 2^31).  Asynchronous on the context's stream, every parameter a kernel argument (capturable).
 * B == 0 or pixels == 0: RN_OK, nothing launched.  RN_ERR_INVALID, nothing launched: ctx, srcs, channels, dst or a
 * source NULL, per_image NULL with channels or channels without per_image, n_src 0 or above 8, a channel count of 0
 * or no multiple of 16 bytes, a pointer off a 16-byte boundary, dst overlapping a source or per_image, an unknown
 * dtype. */
RN_API int rn_concat_channels_forward_dt(rn_ctx *ctx, int dtype, uint64_t n_src, const void *const *srcs,
                                         const uint64_t *channels, const void *per_image /* nullable */,
                                         uint64_t per_image_channels, void *dst, uint64_t B, uint64_t pixels);
/* torchvision's DeepLabHead(in_channels, classes) in eval mode as a second kind of rn_seg_head: every function above
 * but rn_seg_head_create takes either kind, and so do rn_model_forward_segment(_u8).  With a = aspp_channels
 * (torchvision: 256) and the n = n_rates rates (torchvision: 12, 24, 36):
 *   branch 0      Conv1x1(in, a) + BatchNorm + ReLU
 *   branch i      Conv3x3(in, a, padding = dilation = rates[i-1]) + BatchNorm + ReLU, i = 1..n
 *   pooled        global average over h x w, Conv1x1(in, a) + BatchNorm + ReLU on the [B,1,1,in] result, then the same
 *                 value at every pixel (torchvision upsamples the 1x1 map bilinearly: a constant map; here a copy)
 *   concat        branch 0, branches 1..n, pooled: (n + 2) a channels
 *   project       Conv1x1((n + 2) a, a) + BatchNorm + ReLU (+ Dropout, the identity)
 *   head          Conv3x3(a, a, padding 1) + BatchNorm + ReLU, Conv1x1(a, classes) with bias, the upsample above
 * in_channels a multiple of 64 (at most 8192), aspp_channels a multiple of 64 (at most 1024), classes 1..256, n_rates
 * 1..4, every rate 1..RN_CONV_MAX_DILATION; RN_ERR_INVALID otherwise.  Tensors (rn_seg_head_set_tensor; an unknown
 * key or a wrong element count is refused with the key in the message): classifier.0.convs.i.0.weight and
 * classifier.0.convs.i.1.{weight,bias,running_mean,running_var} for i = 0..n; the pooled branch
 * classifier.0.convs.(n+1).1.weight and classifier.0.convs.(n+1).2.{...} (index 0 of that Sequential is the pool);
 * classifier.0.project.0.weight, classifier.0.project.1.{...}; classifier.1.weight, classifier.2.{...};
 * classifier.4.weight, classifier.4.bias.  rn_seg_head_finalize folds every batch-norm (rn_batchnorm2d_fold), packs
 * every weight (rn_conv2d_pack_weight_dt), pads classes to a multiple of 4 like the FCN kind and packs the centre
 * tap weight[:, :, 1, 1] of every dilated branch as a 1x1 panel.
 * A forward is n + 8 launches on public entry points, the folded scale / shift and ReLU in the epilogues: branch 0;
 * branches 1..n (rn_conv2d_dilated_nhwc_forward_dt); the pool (rn_global_avgpool_nhwc_forward_dt); the pooled 1x1
 * (h = w = 1, M = B); the concat above; project; the 3x3; the classifier (fp32 output, shift = bias); the upsample.
 * Scratch, owned and grown like the FCN kind's: per coarse pixel (n + 1) a for the branches, (n + 2) a for the
 * concat and the padded classes in fp32, per image in + a for the pooled vectors; the projected tensor and the 3x3's
 * output live in two branch tensors, which are dead behind the concat.
 * Centre-tap plan: a dilated branch with rate >= h and rate >= w has one tap inside the image for every output
 * pixel, the centre; such a forward runs that branch as the 1x1 contraction on the centre panel -- a ninth of the
 * FLOPs, the same bits.  Decided per forward from h and w.  It is taken only where both routes round the sum at the
 * same places: every bf16 head; an fp32 head only with in_channels == 64 (from 128 on the fp32 3x3 folds its K sum
 * in chunks that cut the centre tap's range elsewhere than the 1x1 does).  rn_seg_head_set_center_tap(hd, 0 | 1),
 * default 1, switches the plan (A/B runs); RN_ERR_INVALID on an FCN head. */
RN_API int rn_seg_head_create_deeplab(rn_ctx *ctx, rn_seg_head **out, uint64_t in_channels, uint64_t aspp_channels,
                                      uint64_t classes, uint64_t n_rates, const uint64_t *rates);
RN_API int rn_seg_head_set_center_tap(rn_seg_head *hd, int on);
/* The label map (and / or the scores) of B images from one forward: exactly the launches and bits of
 * rn_model_forward_outputs -- same sub-batches, parts, front slices, profile records, the classification head
 * included -- plus the head's launches per launch batch (an FCN head: ops "seg_conv1", "seg_conv2", "seg_upsample"
 * of layer "segmentation" in the profile; a DeepLab head: "aspp_conv0", "aspp_conv1" .. "aspp_convN" with the FLOPs
 * of the route that runs, "aspp_pool", "aspp_pool_conv", "aspp_concat", "aspp_project", then those three), queued
 * right behind the last block of layer4 on that block's stream, where
 * the map still sits in its ping-pong arena (as rn_model_forward_maps exports it).  The outputs are at the model's
 * input size: labels [B,H,W] bytes, scores [B,classes,H,W] fp32 (4-byte aligned), device pointers, either may be
 * NULL.  Every part of a launch batch uses its own slice of the head's scratch, which is sized for one sub-batch
 * (it grows with the refusals of rn_seg_head_forward) and is reused by the next sub-batch behind the join of the
 * parts' streams, like the arenas.  A head that also runs on its own (rn_seg_head_forward) on another stream is
 * the caller's to order.  outs may be NULL, as in rn_model_forward_maps.  The request lives for this call only.
 * RN_ERR_INVALID with a text in rn_last_error of the model's context, nothing launched: seg == NULL, a seg that
 * names nothing, misaligned scores, a model or a head that is not finalized, a head whose in_channels is not
 * rn_model_features or whose storage type (dtype) is not the model's.  rn_model_capture, the pipelines and
 * rn_shard_* carry no segmentation. */
typedef struct rn_seg_outputs { uint8_t *labels; float *scores; } rn_seg_outputs;
RN_API int rn_model_forward_segment(rn_model *m, rn_seg_head *hd, const float *input_nchw, uint64_t B,
                                    const rn_model_outputs *outs /* nullable */, const rn_seg_outputs *seg, int mode);
RN_API int rn_model_forward_segment_u8(rn_model *m, rn_seg_head *hd, const uint8_t *input_nhwc, uint64_t B,
                                       const rn_model_outputs *outs, const rn_seg_outputs *seg, int mode);
/* ---- feature pyramid: torchvision's FeaturePyramidNetwork on the stage maps ------------------------------------
 * The top-down step as ONE launch: dst[b,y,x,c] = lat[b,y,x,c] + top[b, iy(y), ix(x), c], all NHWC of `dtype` (fp32
 * or bf16), top [B,h,w,C], lat and dst [B,H,W,C].  lat_nhwc == NULL: the plain nearest upsample
 * (torch.nn.functional.interpolate(mode="nearest", size=(H, W))).  The source index is torch's size= form, per axis
 * n_in -> n_out, output index o:
 *     scale = (float)n_in / (float)n_out                       (one fp32 division, on the host)
 *     i(o)  = min((int)floorf(fl((float)o * scale)), n_in - 1)
 * the product rounded to fp32 on its own, no double precision and no integer shortcut anywhere
 * (ops.upsample_nearest_add_ref restates it in numpy).  Any ratio: 2x, equal sizes (a dilated backbone), odd sizes
 * (7 -> 13 -> 25 -> 50), shrinking.  Arithmetic: fp32 tensors, one fp32 add per element -- bit for bit
 * lat + F.interpolate(top); bf16 tensors, both operands widened, added in fp32 and rounded once to bf16 (nearest
 * even, the rounding of the contraction epilogues); lat == NULL: a copy, NaN payloads and signed zeros kept.
 * Every lane moves 16 bytes along C, so C * element size is a multiple of 16 bytes and every pointer 16-byte
 * aligned; B * H * W and B * h * w below 2^31 (C below 2^31); offsets are 64-bit.  dst may be lat itself (every
 * element is read and written by the same thread); it must not overlap top and must not overlap lat partly.
 * Asynchronous on the context's stream; allocates and uploads nothing, every parameter is a kernel argument
 * (capturable).  B == 0: RN_OK, nothing launched.  RN_ERR_INVALID, nothing launched, rn_last_error names the
 * operand: ctx, top_nhwc or dst_nhwc NULL, a zero size, a bad channel count, a misaligned pointer, a forbidden
 * overlap, an unknown dtype. */
RN_API int rn_upsample_nearest_add_forward_dt(rn_ctx *ctx, int dtype, const void *top_nhwc /* [B,h,w,C] */, uint64_t B,
                                              uint64_t h, uint64_t w, uint64_t C,
                                              const void *lat_nhwc /* [B,H,W,C] or NULL */,
                                              void *dst_nhwc /* [B,H,W,C]; may be lat_nhwc */, uint64_t H, uint64_t W);
/* torchvision's FeaturePyramidNetwork(in_channels_list, out_channels, extra_blocks=LastLevelMaxPool() or None) in
 * eval mode with norm_layer=None, on any NHWC maps, no model needed.  n_levels 1..4, level 0 the finest; every
 * in_channels a multiple of 64 (at most 8192), out_channels (a) a multiple of 64 (at most 1024); extra 0 = no extra
 * block, 1 = the pool; RN_ERR_INVALID otherwise.  No convolution code of its own.
 * Tensors (rn_fpn_set_tensor, fp32 host data, torchvision's keys and shapes; an unknown key or a wrong element count
 * is refused with the key in the message): inner_blocks.i.0.weight [a,in_i,1,1], inner_blocks.i.0.bias [a],
 * layer_blocks.i.0.weight [a,a,3,3], layer_blocks.i.0.bias [a]; the older spelling without the ".0" (inner_blocks.i.weight)
 * names the same tensors.  rn_fpn_set_dtype (before finalize) chooses the storage type of the input maps, the
 * lateral tensors and the weight panels.  rn_fpn_finalize packs every weight (rn_conv2d_pack_weight_dt); a bias is
 * its convolution's shift, with no scale and no ReLU; it needs every tensor.
 * rn_fpn_level_shape: C, H, W of output `level` when the level's input map is h_in x w_in; level == n_levels is the
 * pooled output (h_in, w_in of the coarsest level; RN_ERR_INVALID without the pool).
 * rn_fpn_forward: x_nhwc[i] [B,h[i],w[i],in_i] of the storage type (16-byte aligned) -> out_nchw[i] [B,a,h[i],w[i]]
 * fp32 (4-byte aligned), and with the pool out_nchw[n_levels] [B,a,(h-1)/2+1,(w-1)/2+1] of the coarsest level; NULL
 * = not wanted (not all of them).  Every launch is on a public entry point, on the context's stream:
 *   1. n lateral 1x1 contractions into the neck's scratch, storage type;
 *   2. n - 1 rn_upsample_nearest_add_forward_dt, coarsest first, each in place on the next finer lateral;
 *   3. a 3x3 contraction (padding 1) per wanted level, fp32 output whatever the storage type;
 *   4. with the pool wanted, rn_maxpool2d_nhwc_forward_dt(k = 1, stride 2, padding 0) on the coarsest 3x3 output;
 *   5. one rn_nhwc_to_nchw_dt per wanted output.
 * A level that is not wanted still runs its lateral and its top-down step (finer levels need them) and skips its 3x3
 * and its export; the coarsest 3x3 also runs when only the pool is wanted.  The neck owns its scratch (per level the
 * lateral tensor and the fp32 output, and the pooled tensor); it grows on first use like a segmentation head's:
 * RN_ERR_UNSUPPORTED on a stream that is being captured, RN_ERR_INVALID while a captured graph of the context lives. */
typedef struct rn_fpn rn_fpn;
RN_API int rn_fpn_create(rn_ctx *ctx, rn_fpn **out, uint64_t n_levels, const uint64_t *in_channels,
                         uint64_t out_channels, int extra /* 0 none, 1 pool */);
RN_API int rn_fpn_set_dtype(rn_fpn *fpn, int dtype);
RN_API int rn_fpn_set_tensor(rn_fpn *fpn, const char *key, const float *host_data, uint64_t numel);
RN_API int rn_fpn_finalize(rn_fpn *fpn);
RN_API int rn_fpn_destroy(rn_fpn *fpn);
RN_API int rn_fpn_level_shape(const rn_fpn *fpn, int level, uint64_t h_in, uint64_t w_in, uint64_t *C, uint64_t *H,
                              uint64_t *W);
RN_API int rn_fpn_forward(rn_fpn *fpn, const void *const *x_nhwc, uint64_t B, const uint64_t *h, const uint64_t *w,
                          float *const *out_nchw);
/* The pyramid of B images from one forward (torchvision's resnet_fpn_backbone): exactly the launches and bits of
 * rn_model_forward_outputs -- same sub-batches, parts, front slices, profile records, the classification head
 * included -- plus the neck's.  stages: the n_levels stages (each 1..4, ascending) whose maps are the neck's levels
 * 0 .. n_levels-1.  fpn_out->level[i]: device buffer [B,a,H_i,W_i] fp32 of level i ("0".."3" of torchvision's dict),
 * level[n_levels] the pooled one ("pool"); NULL = not wanted.  The lateral 1x1 of a stage is queued right behind that
 * stage's last block on that block's stream and reads the stage's output in place, where it still sits in its
 * ping-pong arena, so no stage map is ever copied and no arena is added; the rest of the neck is queued behind
 * layer4's last block, where a segmentation head is.  Profile ops of layer "fpn": "fpn_inner<i>" (behind stage i's
 * blocks), then "fpn_topdown<i>" for i = n-1 .. 1 (level i added into level i-1), "fpn_layer<i>", "fpn_pool",
 * "fpn_export<i>" and "fpn_export_pool", with FLOPs and bytes as the segmentation steps have them.  Every part of a
 * launch batch uses its own slice of the neck's scratch, which is sized for one sub-batch and reused by the next
 * behind the join of the parts' streams.  outs may be NULL, as in rn_model_forward_maps.  The request lives for this
 * call only.  Every architecture, both storage types, any input size and dilation, and the byte route.
 * Refused with a text in rn_last_error of the model's context, nothing launched: a NULL or unfinalized neck or model;
 * a neck whose dtype is not the model's or whose context is on another device; stages NULL, not ascending, outside 1..4; an in_channels that is not the
 * stage's C (rn_model_stage_shape); fpn_out NULL or nothing wanted in it; an output off a 4-byte boundary
 * (RN_ERR_INVALID); a bf16 model with RN_FWD_REFERENCE_OPS (RN_ERR_UNSUPPORTED).  rn_model_capture, the pipelines and
 * rn_shard_* carry no pyramid. */
typedef struct rn_fpn_outputs { float *level[5]; } rn_fpn_outputs;   /* levels 0..n-1, then the pool; NULL = not wanted */
RN_API int rn_model_forward_fpn(rn_model *m, rn_fpn *fpn, const float *input_nchw, uint64_t B,
                                const rn_model_outputs *outs /* nullable */, const int *stages,
                                const rn_fpn_outputs *fpn_out, int mode);
RN_API int rn_model_forward_fpn_u8(rn_model *m, rn_fpn *fpn, const uint8_t *input_nhwc, uint64_t B,
                                   const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                                   int mode);
/* ---- RoIAlign over the pyramid: torchvision's MultiScaleRoIAlign as ONE launch ---------------------------------
 * rn_roi_align_forward_dt pools K regions from n_levels NHWC maps (1..4, finest first; x_nhwc[i] [B,h[i],w[i],C] of
 * `dtype`, 16-byte aligned, C * element size a multiple of 16 bytes, scales[i] its spatial scale) into
 * out [K,C,PH,PW] fp32 (torchvision's layout, 4-byte aligned); every RoI picks its level inside the kernel.
 * rois_dev: device [K,5] fp32 (image index, x1, y1, x2, y2) in input-image pixels, torchvision's format.
 * levels_out: the chosen level of every RoI, int32 [K], or NULL.  PH, PW 1..32; sampling_ratio 1..4 (<= 0, the
 * adaptive grid, is RN_ERR_UNSUPPORTED); aligned 0 or 1.
 * The arithmetic is a contract, torchvision's roi_align in its own order; every operation fp32 and rounded on its
 * own, none fused (ops.roi_align_ref restates it in numpy).  With S = sampling_ratio, h x w the level's map:
 *   extent:  off = aligned ? 0.5 : 0;  x1s = x1 * scale - off, likewise y1s, x2s, y2s;  rw = x2s - x1s, rh = y2s - y1s,
 *            each replaced by 1 where it is < 1 and not aligned;  bin_h = rh / PH, bin_w = rw / PW.
 *   sample:  y = y1s + ph * bin_h + (iy + 0.5) * bin_h / S (the product before the quotient), x likewise.
 *            It contributes only if y >= -1 && y <= h && x >= -1 && x <= w (a NaN coordinate contributes nothing).
 *            Then y = max(y, 0), yl = (int)y; if yl >= h - 1: yl = yh = h - 1, y = yl; else yh = yl + 1; x likewise;
 *            ly = y - yl, hy = 1 - ly, lx, hx likewise;
 *            val = hy*hx*v1 + hy*lx*v2 + ly*hx*v3 + ly*lx*v4, added left to right (v1 = (yl,xl), v2 = (yl,xh),
 *            v3 = (yh,xl), v4 = (yh,xh)); a bf16 value is widened exactly.
 *   bin:     the samples summed with iy outer and ix inner, the sum divided by S * S.
 * The index clamps are unconditional: no RoI content (NaN, +-Inf, 1e30) indexes outside its map.  A RoI whose image
 * index is not an integer in [0, B) gets a row of zeros and level -1.
 * Level: area = (x2 - x1) * (y2 - y1) in fp32, image pixels; level = the number of j with area >= thr[j], thr the
 * n_levels - 1 thresholds of rn_roi_level_thresholds (host only): k_min = round(-log2(scales[0])),
 * thr[j] = (canonical_scale * 2^(k_min + 1 + j - canonical_level - 1e-6))^2 in double, rounded up to fp32 -- the
 * boundaries of torchvision's LevelMapper floor(k0 + log2(sqrt(area) / s0) + 1e-6) clamped to the levels (defaults
 * s0 = 224, k0 = 4), with no logarithm on the device.
 * One block takes one RoI and a slab of channels; the slab's outputs are one contiguous run of `out`, stored by
 * rn_nhwc_to_nchw_dt's rule.  Offsets are 64-bit; B * h * w, C, B and K below 2^31.  Asynchronous on the context's
 * stream; allocates and uploads nothing (capturable).  K == 0 or B == 0: RN_OK, nothing launched.  RN_ERR_INVALID,
 * nothing launched, rn_last_error names the operand: a NULL pointer, a misaligned pointer, a bad C, a parameter out
 * of range, a size at or above 2^31, a scale that is not positive and finite, out or levels_out overlapping an input
 * or each other. */
RN_API int rn_roi_level_thresholds(uint64_t n_levels, const float *scales, double canonical_scale, int canonical_level,
                                   float *thr_out /* n_levels - 1 */);
RN_API int rn_roi_align_forward_dt(rn_ctx *ctx, int dtype, uint64_t n_levels, const void *const *x_nhwc, const uint64_t *h,
                                   const uint64_t *w, const float *scales, const float *thr, uint64_t B, uint64_t C,
                                   const float *rois_dev, uint64_t K, uint64_t PH, uint64_t PW, int sampling_ratio,
                                   int aligned, float *out, int32_t *levels_out /* nullable */);
/* A pooler behind a neck: the RoIs (device, [K,5]), the size of the input image they are given in, the neck's levels
 * the pooler reads (ascending, 0 .. n_levels - 1 of the neck; the pooled extra level is none of them), the pooler's
 * parameters and the outputs: pooled [K,a,PH,PW] fp32 and, optionally, levels_out int32 [K] (indices into `level`).
 * The scale of a level is torchvision's, 2^round(log2(h_level / image_h)), computed on the host (the height's, as
 * torchvision returns it).  The kernel reads the fp32 3x3 outputs in the neck's scratch in place, so the neck runs the
 * 3x3 of every level the pooler reads, exported or not.
 * rn_fpn_forward_rois: rn_fpn_forward plus the pooler, queued last; out_nchw may be NULL (no level exported).
 * rn_model_forward_rois(_u8): rn_model_forward_fpn(_u8)'s launches plus the pooler, queued behind the neck's last
 * launch of every part with the profile op "roi_align" of layer "fpn"; fpn_out may be NULL.  Every part of a launch
 * batch pools the RoIs of its own images from its own slice of the scratch; every row of `pooled` is written exactly
 * once per forward (rows of an invalid image index by the part that holds image 0).  The pooler follows the neck:
 * dtype, input size, dilation, every architecture, the byte route.  Refused like rn_model_forward_fpn, and: a level
 * that is not the neck's, rois_dev or pooled NULL with K > 0, a parameter out of range, pooled, levels_out or
 * rois_dev sharing a byte with each other, an exported level or a head output of the call (RN_ERR_INVALID),
 * sampling_ratio <= 0 (RN_ERR_UNSUPPORTED).  rn_model_capture, the pipelines and rn_shard_* carry no pooler. */
typedef struct rn_roi_pool {
    const float *rois_dev;
    uint64_t K, image_h, image_w;
    int n_levels, level[4];
    uint64_t PH, PW;
    int sampling_ratio, aligned;
    double canonical_scale; /* 224 */
    int canonical_level;    /* 4 */
    float *pooled;
    int32_t *levels_out; /* nullable */
} rn_roi_pool;
RN_API int rn_fpn_forward_rois(rn_fpn *fpn, const void *const *x_nhwc, uint64_t B, const uint64_t *h, const uint64_t *w,
                               float *const *out_nchw /* nullable */, const rn_roi_pool *rois);
RN_API int rn_model_forward_rois(rn_model *m, rn_fpn *fpn, const float *input_nchw, uint64_t B,
                                 const rn_model_outputs *outs /* nullable */, const int *stages,
                                 const rn_fpn_outputs *fpn_out /* nullable */, const rn_roi_pool *rois, int mode);
RN_API int rn_model_forward_rois_u8(rn_model *m, rn_fpn *fpn, const uint8_t *input_nhwc, uint64_t B,
                                    const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                                    const rn_roi_pool *rois, int mode);
/* ---- RPN proposals behind the head: top-k, box decode, NMS and the merge over the levels (rn_rpn.hip) ----------
 * torchvision's RegionProposalNetwork in eval mode behind RPNHead (AnchorGenerator, BoxCoder.decode,
 * filter_proposals), as three launches: rn_rpn_select_decode_forward (one) and rn_rpn_nms_merge_forward (two: the IoU
 * mask, then the scan and the merge).  The arithmetic is a contract; every fp32 operation is rounded on its own and
 * none is fused (rpn.py restates it in numpy).  min(a, b) is a > b ? b : a and max(a, b) is a < b ? b : a: a NaN in
 * `a` stays.  L = 1..5 levels, finest first; A = 1..12 anchors per position, the same on every level; the image is
 * H x W, a level h x w.
 *   Anchors:  per level, sizes s_j and ratios r_i; hr = sqrtf(r), wr = 1 / hr; base anchor (i, j), at index
 *             i * n_sizes + j, is rint((-wr*s, -hr*s, wr*s, hr*s) / 2), half to even, formed on the host in fp32:
 *             base_anchors is that table, [L, A, 4].  Strides sh = H / h, sw = W / w, INTEGER division.  Anchor
 *             n = (y*w + x)*A + a is base[a] + (x*sw, y*sh, x*sw, y*sh).
 *   Head:     per level NHWC fp32 [B, h, w, P], P = 5A rounded up to a multiple of 4; channel a is the objectness
 *             logit of anchor a, channel A + 4a + c is delta c of anchor a (torchvision's permute_and_flatten order).
 *   Select:   per (image, level) the min(pre_nms_top_n, h*w*A) first anchors in rn_topk_forward's order: (v_i, i)
 *             precedes (v_j, j) when v_i > v_j, or v_i == v_j and i < j; -0 == +0 and a NaN ranks as -inf.
 *   Decode:   weights wx, wy, ww, wh (the RPN's: 1, 1, 1, 1), clip = (float)log(1000.0 / 16.0):
 *             wa = ax2 - ax1; cx = ax1 + 0.5f*wa; dx = d0 / wx; dw = min(d2 / ww, clip); pcx = dx*wa + cx;
 *             pw = expf(dw)*wa; x1 = pcx - 0.5f*pw; x2 = pcx + 0.5f*pw; y likewise (ha, cy, d1 / wy, d3 / wh);
 *             then x = min(max(x, 0), W), y = min(max(y, 0), H).  expf is the device's: the one operation that is not
 *             bit-defined against numpy.
 *   Valid:    (x2 - x1 >= min_size) && (y2 - y1 >= min_size) && (logit >= logit_thresh); a NaN anywhere fails.
 *             logit_thresh is logit(score_thresh) formed by the caller (score_thresh 0: -INFINITY).  Scores are
 *             logits end to end.
 *   NMS:      per segment, on candidates in their given order; an invalid candidate neither survives nor suppresses;
 *             candidate i survives if no surviving j < i has inter / (area_i + area_j - inter) > nms_thresh, with
 *             inter = max(min(x2i,x2j) - max(x1i,x1j), 0) * max(min(y2i,y2j) - max(y1i,y1j), 0) and
 *             area = (x2 - x1) * (y2 - y1); 0/0 is a NaN and does not suppress.  (torchvision's nms on the unshifted
 *             boxes of a level, _batched_nms_vanilla; not the coordinate-offset form of batched_nms.)
 *   Merge:    per image the survivors of all levels in the order of (logit, position), position = level *
 *             pre_nms_top_n + rank, the same order as Select; the first post_nms_top_n are the proposals.
 * rn_rpn_candidates, per (image, level, rank) [B, L, pre_nms_top_n]: index int32 (the anchor n), logit, box [.., 4],
 * valid (bytes 0 / 1) and count [B, L] int32 (min(pre_nms_top_n, h*w*A)); ranks at or past count hold index -1,
 * logit -inf, box 0, valid 0.  rn_rpn_select_decode_forward writes those that are not NULL (not all may be), every
 * row on every call.
 * rn_rpn_proposals: boxes [B, post, 4], logits [B, post], levels [B, post] int32, count [B] int32, rois [B*post, 5]
 * in the pooler's format (image index, x1, y1, x2, y2), cand_keep [B, L, pre] bytes (the candidates NMS left); any
 * may be NULL, not all.  Rows at or past an image's count hold boxes 0, logit -inf, level -1 and RoI image index -1
 * (the pooler answers such a row with zeros and level -1).  Every row is written on every call.
 * rn_nms_forward: S segments of n <= 4096 boxes [S, n, 4], already in score order, valid [S, n] bytes or NULL (all
 * valid) -> keep [S, n] bytes, keep_count [S] int32 or NULL.  Two launches: mask and scan.
 * rn_box_decode_forward: Decode on its own, anchors [N, 4] + deltas [N, 4] -> boxes [N, 4], one launch; image_h and
 * image_w are the clip's H and W (INFINITY: no upper clip).  A second-stage box head uses weights (10, 10, 5, 5).
 * The IoU mask (one 64-bit word per candidate row and block of 64 columns, upper triangle only, vector stores) lives
 * in a scratch of the context that grows on demand: never during a capture, not while a captured graph lives.  No
 * floating-point atomics and no atomics on global memory anywhere.  All asynchronous on the context's stream; the
 * launch counts do not depend on B or S.  B, S or N == 0: RN_OK, nothing launched.  RN_ERR_INVALID, nothing launched,
 * rn_last_error names the operand: a NULL operand, an operand of 4-byte elements off a 4-byte boundary, an output
 * sharing a byte with another operand, a parameter out of range (pre_nms_top_n, post_nms_top_n 1..4096; h*w*A below
 * 2^31; B, B*L and S at most 65535; a NaN threshold). */
typedef struct rn_rpn_candidates {
    int32_t *index;
    float *logit;
    float *box;
    uint8_t *valid;
    int32_t *count;
} rn_rpn_candidates;
typedef struct rn_rpn_proposals {
    float *boxes;
    float *logits;
    int32_t *levels;
    int32_t *count;
    float *rois;
    uint8_t *cand_keep;
} rn_rpn_proposals;
RN_API int rn_rpn_select_decode_forward(rn_ctx *ctx, uint64_t L, const float *const *head_nhwc, uint64_t B,
                                        const uint64_t *h, const uint64_t *w, uint64_t A,
                                        const float *base_anchors /* host, [L, A, 4] */, uint64_t image_h,
                                        uint64_t image_w, uint64_t pre_nms_top_n, float min_size, float logit_thresh,
                                        const rn_rpn_candidates *cand);
RN_API int rn_rpn_nms_merge_forward(rn_ctx *ctx, const rn_rpn_candidates *cand, uint64_t B, uint64_t L,
                                    uint64_t pre_nms_top_n, uint64_t post_nms_top_n, float nms_thresh,
                                    const rn_rpn_proposals *out);
RN_API int rn_nms_forward(rn_ctx *ctx, const float *boxes, const uint8_t *valid /* nullable */, uint64_t S, uint64_t n,
                          float iou_threshold, uint8_t *keep, int32_t *keep_count /* nullable */);
RN_API int rn_box_decode_forward(rn_ctx *ctx, const float *anchors, const float *deltas, uint64_t N, float wx, float wy,
                                 float ww, float wh, float image_h, float image_w, float *boxes);
/* The RPN as an object, modelled on rn_fpn: torchvision's RPNHead (3x3 C -> C with ReLU, then cls_logits and bbox_pred as
 * ONE 1x1 C -> P panel, zero rows up to P, the biases as the epilogues' shifts: exact) in front of the three launches.
 * rn_rpn_create(ctx, &rpn, in_channels (a multiple of 64), L, A, base_anchors [L, A, 4] host); rn_rpn_set_tensor takes
 * "head.conv.0.0.weight|bias" (older spelling "head.conv.weight|bias"), "head.cls_logits.weight|bias",
 * "head.bbox_pred.weight|bias" (host fp32); rn_rpn_finalize packs the two panels.  rn_rpn_forward runs the stage on
 * caller-given fp32 NHWC levels x_nhwc[l] [B, h[l], w[l], in_channels] (16-byte aligned) of an image_h x image_w image:
 * 2 L + 3 launches whatever B (two contractions per level, select + decode, mask, scan + merge).  The request: the
 * parameters, the proposals' outputs (any may be NULL, not all) and the optional pre-NMS candidates (all may be NULL).
 * The object's scratch (head outputs, candidates, mask) grows on demand: never during a capture, not while a captured
 * graph lives.  Refused (RN_ERR_INVALID, nothing launched, rn_last_error names the operand): as the stand-alone ops,
 * and an output sharing a byte with a level's map.
 * rn_fpn_forward_proposals: rn_fpn_forward plus the stage on the neck's fp32 3x3 outputs and pooled level, read in
 * place (so the 3x3 of every level runs, exported or not); the rpn's L is the neck's levels plus its pool.  Queued after
 * the exports and before the pooler.  rois (nullable): a pooler as in rn_fpn_forward_rois; when rois->rois_dev ==
 * req->out.rois and rois->K == B * post_nms_top_n the pooler pools the proposals of the same call -- the only case in
 * which rois_dev may be an output of the call; the padding rows give zeros and level -1. */
typedef struct rn_rpn rn_rpn;
typedef struct rn_rpn_request {
    uint64_t pre_nms_top_n, post_nms_top_n;
    float nms_thresh, logit_thresh, min_size;
    rn_rpn_proposals out;
    rn_rpn_candidates cand; /* optional */
} rn_rpn_request;
RN_API int rn_rpn_create(rn_ctx *ctx, rn_rpn **out, uint64_t in_channels, uint64_t L, uint64_t A, const float *base_anchors);
RN_API int rn_rpn_set_tensor(rn_rpn *rpn, const char *key, const float *host_data, uint64_t numel);
RN_API int rn_rpn_finalize(rn_rpn *rpn);
RN_API int rn_rpn_destroy(rn_rpn *rpn);
RN_API int rn_rpn_forward(rn_rpn *rpn, const float *const *x_nhwc, uint64_t B, const uint64_t *h, const uint64_t *w,
                          uint64_t image_h, uint64_t image_w, const rn_rpn_request *req);
RN_API int rn_fpn_forward_proposals(rn_fpn *fpn, rn_rpn *rpn, const void *const *x_nhwc, uint64_t B, const uint64_t *h,
                                    const uint64_t *w, float *const *out_nchw /* nullable */, uint64_t image_h,
                                    uint64_t image_w, const rn_rpn_request *req, const rn_roi_pool *rois /* nullable */);
/* rn_model_forward_proposals(_u8): rn_model_forward_rois(_u8)'s arguments plus the rpn and its request; the pooler is
 * nullable.  The image size is the model's input size.  Every part of a launch batch runs the stage on its own images
 * from its own slice of the neck's and the rpn's scratch and writes its own rows, after the exports and before the
 * pooler (one profile record "rpn_stage" of layer "rpn").  With the chain (rois->rois_dev == req->out.rois and K == B *
 * post_nms_top_n) the pooler of a part takes exactly its own images' rows of the RoIs, pooled and levels_out, padding
 * rows included, so no part reads a row another part has yet to write.  Refused like rn_model_forward_rois, and: an rpn
 * that is not the neck's, a request out of range, an output of the request sharing a byte with another output of the
 * call. */
RN_API int rn_model_forward_proposals(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, const float *input_nchw, uint64_t B,
                                      const rn_model_outputs *outs /* nullable */, const int *stages,
                                      const rn_fpn_outputs *fpn_out /* nullable */, const rn_rpn_request *req,
                                      const rn_roi_pool *rois /* nullable */, int mode);
RN_API int rn_model_forward_proposals_u8(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, const uint8_t *input_nhwc, uint64_t B,
                                         const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                                         const rn_rpn_request *req, const rn_roi_pool *rois, int mode);
/* ---- The box head behind the pooler: FC layers, class scores, per-class NMS, the merge (rn_detect.hip) ----------------
 * torchvision's TwoMLPHead, FastRCNNPredictor and RoIHeads.postprocess_detections in eval mode.  The post-processing
 * is rn_detect_postprocess_forward: THREE launches whatever B, R and C (score + decode; per-class sort + NMS; merge).
 * The arithmetic is a contract, restated in numpy in detection.py; every fp32 operation is rounded on its own and none
 * is fused; min and max are the RPN section's.  B images; R = 1..4096 RoIs per image; K = B*R rows, image b owns rows
 * b*R .. b*R + R - 1 (rn_rpn_proposals.rois with R = post_nms_top_n); C = 2..1024 classes, background 0 included;
 * D = detections_per_img = 1..1024.
 *   Head:     [K, P] fp32, P = 5C rounded up to a multiple of 4; column c is the logit of class c, column C + 4c + j
 *             delta j of class c (torchvision's bbox_pred row 4c + j).
 *   Score:    p[k][c] is rn_softmax_forward's probability of the C logits of row k, bit for bit: the launch has that
 *             kernel's block shape and shares its statistics' code (one max, one summation order, one division).
 *   Decode:   for c >= 1 the RPN section's Decode of RoI k's box (x1, y1, x2, y2) with class c's deltas and the
 *             request's weights (torchvision: 10, 10, 5, 5); the clip constant and the clamp to W, H are unchanged;
 *             expf stays the one operation that is not bit-defined.
 *   Valid:    the row is real (its RoI image index equals b; the RPN's padding rows carry -1) && p > score_thresh
 *             (STRICT, as torchvision) && x2 - x1 >= min_size && y2 - y1 >= min_size (torchvision: 1e-2); a NaN
 *             anywhere fails.  Class 0 is never valid.
 *   NMS:      per (image, class c >= 1) the valid candidates in the order (p descending, r ascending), -0 == +0, and
 *             on them the NMS of the RPN section.  This is torchvision's nms on the unshifted boxes of a class
 *             (_batched_nms_vanilla); it is NOT the coordinate-offset form batched_nms takes below 4000 boxes, whose
 *             shifted coordinates round differently.
 *   Merge:    per image the survivors of all classes in the order (p descending, f ascending), f = r*(C-1) + (c-1)
 *             (torchvision's flattened index after it drops the background column); the first D are the detections.
 * rn_detections: boxes [B,D,4], scores [B,D], labels [B,D] int32, roi [B,D] int32 (the row r a detection came from),
 * count [B] int32; any may be NULL, not all five.  Rows at or past count hold box 0, score 0, label -1, roi -1.
 * Optional intermediates, row-major by RoI: probs [K,C], class_boxes [K,C,4], valid [K,C] bytes, keep [K,C] bytes (the
 * candidates NMS left); column 0 is written as box 0, valid 0, keep 0.  Every row of every output that is not NULL is
 * written on every call.
 * Scratch is O(B*C*R) -- 12 bytes per (RoI, class), the class boxes where the caller does not take them, a count per
 * (image, class); there is no IoU mask -- in the context's scratch, which grows on demand: never during a capture, not
 * while a captured graph lives.  No floating-point atomics and no atomics on global memory.  Asynchronous on the
 * context's stream.  B == 0: RN_OK, nothing launched.  RN_ERR_INVALID, nothing launched, rn_last_error names the
 * operand: a NULL operand, an operand of 4-byte elements off a 4-byte boundary, an output sharing a byte with another
 * operand, a parameter out of range (R, C, D as above; B at most 65535; B*R below 2^31; image_h, image_w 1 .. 2^24 - 1;
 * weights positive and finite), a NaN threshold. */
typedef struct rn_detections {
    float *boxes;
    float *scores;
    int32_t *labels;
    int32_t *roi;
    int32_t *count;
    float *probs;       /* optional intermediates from here on */
    float *class_boxes;
    uint8_t *valid;
    uint8_t *keep;
} rn_detections;
typedef struct rn_detect_request {
    float score_thresh, nms_thresh, min_size;
    uint64_t detections_per_img;
    float weights[4]; /* wx, wy, ww, wh */
    rn_detections out;
} rn_detect_request;
RN_API int rn_detect_postprocess_forward(rn_ctx *ctx, const float *head /* [K,P] */, const float *rois /* [K,5] */,
                                         uint64_t B, uint64_t R, uint64_t C, uint64_t image_h, uint64_t image_w,
                                         const rn_detect_request *req);
/* The box head as an object, modelled on rn_rpn: rn_box_head_create(ctx, &bh, in_features = a*PH*PW, representation
 * (both multiples of 64), classes); rn_box_head_set_tensor takes "box_head.fc6.weight|bias", "box_head.fc7.weight|bias",
 * "box_predictor.cls_score.weight|bias", "box_predictor.bbox_pred.weight|bias" (host fp32, torch.nn.Linear's [out, in]);
 * rn_box_head_finalize packs three 1x1 panels: fc6, fc7 and ONE panel of cls_score with bbox_pred and zero rows up to P;
 * the biases are the epilogues' shifts and ReLU sits on fc6 and fc7: exact.  rn_box_head_forward runs three contractions
 * and the three launches above on pooled [K, a, PH, PW] fp32 (16-byte aligned), which already is the row-major
 * [K, in_features] matrix in torchvision's flatten(1) order: read in place, no transpose, no copy.  fp32 only.  A contraction is one
 * launch, or two where its plan finishes a chunked K sum in a second pass (few rows under a long K), so a forward is 6 to
 * 9 launches: the count depends on the contraction's plan for (K rows, in_features, representation), never on B, R or C
 * behind the head.
 * head_out (nullable): the head output [K, P], copied out of the object's scratch.  The scratch (the FC outputs, the head
 * output, the stage's) grows on demand: never during a capture, not while a captured graph lives.  Refused as the
 * stand-alone op, and: an output sharing a byte with pooled, rois or head_out. */
typedef struct rn_box_head rn_box_head;
RN_API int rn_box_head_create(rn_ctx *ctx, rn_box_head **out, uint64_t in_features, uint64_t representation,
                              uint64_t classes);
RN_API int rn_box_head_set_tensor(rn_box_head *bh, const char *key, const float *host_data, uint64_t numel);
RN_API int rn_box_head_finalize(rn_box_head *bh);
RN_API int rn_box_head_destroy(rn_box_head *bh);
RN_API int rn_box_head_forward(rn_box_head *bh, const float *pooled, const float *rois, uint64_t B, uint64_t R,
                               uint64_t image_h, uint64_t image_w, const rn_detect_request *req,
                               float *head_out /* nullable */);
/* The box head behind the neck and inside a forward.  rn_fpn_forward_detections: rn_fpn_forward_proposals plus the box
 * head and its request; rn_model_forward_detections(_u8): rn_model_forward_proposals(_u8)'s arguments plus them.  Both
 * require the chained pooler (rois->rois_dev == req->out.rois and rois->K == B * post_nms_top_n) and a pooled on a
 * 16-byte boundary; R is post_nms_top_n and the image the neck call's image_h x image_w resp. the model's input size.
 * Each part of a launch batch runs the head on exactly its own rows of pooled and of the RoIs, behind its own pooler
 * launch, from its own slice of the box head's scratch, and writes its own [b] rows (one profile record "box_stage" of
 * layer "roi_heads").  Refused like the proposals' calls, and: a box head whose in_features is not a * PH * PW, a
 * request out of range, an output of the request sharing a byte with any other output of the call (the rpn's, the
 * pooler's, an exported level, a head output).  Every other forward kind issues exactly the launches it issued. */
RN_API int rn_fpn_forward_detections(rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, const void *const *x_nhwc, uint64_t B,
                                     const uint64_t *h, const uint64_t *w, float *const *out_nchw /* nullable */,
                                     uint64_t image_h, uint64_t image_w, const rn_rpn_request *req,
                                     const rn_roi_pool *rois, const rn_detect_request *det_req);
RN_API int rn_model_forward_detections(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, const float *input_nchw,
                                       uint64_t B, const rn_model_outputs *outs /* nullable */, const int *stages,
                                       const rn_fpn_outputs *fpn_out /* nullable */, const rn_rpn_request *req,
                                       const rn_roi_pool *rois, const rn_detect_request *det_req, int mode);
RN_API int rn_model_forward_detections_u8(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, const uint8_t *input_nhwc,
                                          uint64_t B, const rn_model_outputs *outs, const int *stages,
                                          const rn_fpn_outputs *fpn_out, const rn_rpn_request *req,
                                          const rn_roi_pool *rois, const rn_detect_request *det_req, int mode);
/* ---- The mask head behind the box head: convs, deconv, class select and paste (rn_mask.hip; the pooler form: rn_roi.hip) --
 * torchvision's mask branch of RoIHeads in eval mode: mask_roi_pool on the DETECTED boxes, MaskRCNNHeads (3x3
 * convolutions with bias and ReLU), MaskRCNNPredictor (conv5_mask, a ConvTranspose2d(., Cr, 2, 2) with ReLU, then the 1x1
 * mask_fcn_logits), maskrcnn_inference (the sigmoid of the channel of each detection's own label) and
 * paste_masks_in_image.  fp32 only, like the box head.  Every entry point is asynchronous on the context's stream and
 * allocates nothing outside scratch that grows on demand; none of its kernels uses an atomic.  No content of a label or
 * a box indexes outside a buffer: the index clamps are unconditional.  Refusals: RN_ERR_INVALID, nothing launched,
 * rn_last_error names the operand; no output may share a byte with another operand; K, B or D == 0: RN_OK, nothing
 * launched.
 *
 * rn_roi_align_nhwc_forward_dt: rn_roi_align_forward_dt with the output as [K, PH, PW, C], the layout the convolutions
 * read.  Every argument, every refusal and every value are that function's: element (k, ph, pw, c) holds, bit for bit,
 * its (k, c, ph, pw), the rows of zeros and the level -1 of an invalid image index included.  out_nhwc sits on a 16-byte
 * boundary: a thread stores the 4 (bf16 maps: 8) channels it summed with 16-byte stores, no LDS transposition.
 *
 * rn_detection_rois_forward: boxes [B,D,4] fp32 and labels [B,D] int32 (device) -> rois [B*D,5]: row (b, d) is
 * (b, x1, y1, x2, y2) where labels[b][d] >= 1 and (-1, 0, 0, 0, 0) otherwise -- the padding rows of rn_detections carry
 * label -1, and the pooler answers an image index of -1 with zeros.  One launch, 16-byte stores wherever four
 * consecutive outputs share an aligned 16 bytes.  B * D * 5 below 2^31.
 *
 * rn_mask_predict_forward: t [K, M, M, 4*Cr] fp32 on a 16-byte boundary, the deconvolution's output after bias and ReLU
 * with channel (dy*2 + dx)*Cr + c holding output pixel (2y + dy, 2x + dx), channel c; labels [K] int32; weight [C, Cr]
 * (16-byte aligned) and bias [C] fp32 on the device, mask_fcn_logits in torchvision's layout -> probs [K, 2M, 2M] fp32:
 *     probs[k][2y+dy][2x+dx] = 1 / (1 + expf(-(bias[l] + sum_c weight[l][c] * t[k][y][x][(dy*2+dx)*Cr + c]))), l = labels[k]
 * and a row whose label is outside [1, C) is all zeros.  Only the label's row of the 1x1 is computed; no [K, C, 2M, 2M]
 * tensor exists.  Cr a multiple of 64 up to 1024, M 1..32, C 2..1024.  The sum is not bit-defined against numpy and
 * neither is expf, but the order is fixed: with j = c / 4, lane li = j % 16 adds its products to 0 in ascending c, and
 * the sixteen partial sums fold by the butterfly 8, 4, 2, 1 (lane li takes li ^ 8, then ^ 4, ^ 2, ^ 1).  It depends on
 * Cr alone -- not on K, the row's position or a launch's window -- so a row computed inside a model's forward carries
 * the bits of the stand-alone run.
 *
 * rn_paste_masks_forward: paste_masks_in_image with padding 1.  probs [K, Mo, Mo] fp32 (Mo 1..64), boxes [K, 4] fp32,
 * labels [K] int32 or NULL (all valid), the image H x W (each below 2^24, H * W below 2^31 - 8192), threshold ->
 * masks [K, H, W] fp32 (4-byte aligned) and / or bits [K, H, W] bytes (anywhere) holding mask > threshold; either may be
 * NULL, not both.  Every byte is written exactly once, with 16-byte (bits: 4-byte) stores wherever four consecutive
 * outputs share an aligned unit, whatever W and the addresses are (rn_upsample_bilinear_forward's rule; scalars remain
 * where a wave's last lane has no neighbour and at a plane's ends).  The arithmetic is torchvision's, every fp32
 * operation rounded on its own (mask.paste_masks_ref restates it in numpy; the kernel matches it bit for bit):
 *     s  = (float)((double)(Mo + 2) / (double)Mo)                                   (host)
 *     wh = ((x2 - x1) * 0.5f) * s;  hh likewise;  xc = (x2 + x1) * 0.5f;  yc likewise
 *     bx0 = (int)(xc - wh), by0 = (int)(yc - hh), bx1 = (int)(xc + wh), by1 = (int)(yc + hh)    truncation toward zero,
 *                                                                    each clamped to +-2^30 before the conversion
 *     w = max(bx1 - bx0 + 1, 1);  h = max(by1 - by0 + 1, 1)
 *     pixel (y, x) with max(bx0,0) <= x < min(bx1+1, W) and max(by0,0) <= y < min(by1+1, H):
 *         the bilinear value (align_corners = False) of the zero-padded (Mo+2) x (Mo+2) map resized to h x w at
 *         (y - by0, x - bx0), by the per-axis rule and the sum order of rn_upsample_bilinear_forward's contract, with
 *         scale = (float)(Mo+2) / (float)w  resp.  / (float)h   (one fp32 division, here on the device)
 *     every other pixel: 0
 * A row is all zeros when its label is below 1 (where labels is given), when its box has a non-finite coordinate, or
 * when one of the four expanded coordinates xc -+ wh, yc -+ hh is not finite (the expansion of a box near FLT_MAX).
 * One block holds one detection's padded map in LDS and 8192 consecutive outputs of its plane; a block none of whose
 * rows meets the box reads nothing.
 *
 * The object.  rn_mask_head_create(ctx, &mh, in_channels, n_layers (1..8), layer_channels[], dim_reduced, classes,
 * resolution M (1..32)); channel counts are multiples of 64 (dim_reduced at most 1024).  rn_mask_head_set_tensor takes
 * host fp32 in both spellings of torchvision, with or without the "roi_heads." prefix: mask_head.{i}.0.weight|bias and
 * mask_head.mask_fcn{i+1}.weight|bias ([c_i, c_{i-1}, 3, 3], [c_i]), mask_predictor.conv5_mask.weight|bias
 * ([c_last, Cr, 2, 2], [Cr]), mask_predictor.mask_fcn_logits.weight|bias ([C, Cr, 1, 1], [C]).  rn_mask_head_finalize
 * needs every tensor; it packs each 3x3 through rn_conv2d_pack_weight_dt (the bias is the epilogue's shift, ReLU on) and
 * the transposed convolution as ONE 1x1 panel of 4*Cr output channels, row (dy*2+dx)*Cr + co = W[:, co, dy, dx], the
 * shift the bias four times, ReLU on: exact, because kernel 2 at stride 2 overlaps nothing.  norm_layer and dilation of
 * MaskRCNNHeads are not carried.
 * rn_mask_head_forward: pooled_nhwc [K, M, M, in_channels] fp32 (16-byte aligned), labels [K], boxes [K, 4] (NULL: no
 * paste, masks and bits of the request must be NULL), the image size and the request -> n_layers + 1 contractions
 * (rn_conv2d_nhwc_forward_dt: one launch each, or two where the plan finishes a chunked K sum in a second pass), the
 * predict launch, the paste launch where masks or bits is wanted.  Of the request it reads threshold, probs [K, 2M, 2M],
 * masks and bits [K, H, W] (any may be NULL, not all three); the pooler's parameters, rois and pooled are the route's.
 * The scratch -- two ping-pong maps, the [K, M, M, 4*Cr] tensor and the probabilities of a forward that does not export
 * them -- grows on demand, never on a stream that is being captured and never while a captured graph of the context lives. */
typedef struct rn_mask_request {
    int n_levels, level[4];            /* the mask pooler's levels of the neck, as rn_roi_pool's */
    int sampling_ratio, aligned;
    double canonical_scale;            /* 224 */
    int canonical_level;               /* 4 */
    float threshold;                   /* bits = mask > threshold; torchvision: 0.5 */
    float *rois;                       /* [B*D, 5] or NULL */
    float *pooled;                     /* [B*D, M, M, a] or NULL */
    float *probs;                      /* [B, D, 2M, 2M] or NULL */
    float *masks;                      /* [B, D, H, W] or NULL */
    uint8_t *bits;                     /* [B, D, H, W] or NULL */
} rn_mask_request;
typedef struct rn_mask_head rn_mask_head;
RN_API int rn_roi_align_nhwc_forward_dt(rn_ctx *ctx, int dtype, uint64_t n_levels, const void *const *x_nhwc,
                                        const uint64_t *h, const uint64_t *w, const float *scales, const float *thr,
                                        uint64_t B, uint64_t C, const float *rois_dev, uint64_t K, uint64_t PH, uint64_t PW,
                                        int sampling_ratio, int aligned, float *out_nhwc, int32_t *levels_out /* nullable */);
RN_API int rn_detection_rois_forward(rn_ctx *ctx, const float *boxes, const int32_t *labels, uint64_t B, uint64_t D,
                                     float *rois);
RN_API int rn_mask_predict_forward(rn_ctx *ctx, const float *t, const int32_t *labels, const float *weight,
                                   const float *bias, uint64_t K, uint64_t M, uint64_t Cr, uint64_t C, float *probs);
RN_API int rn_paste_masks_forward(rn_ctx *ctx, const float *probs, const float *boxes, const int32_t *labels /* nullable */,
                                  uint64_t K, uint64_t Mo, uint64_t H, uint64_t W, float threshold,
                                  float *masks /* nullable */, uint8_t *bits /* nullable */);
RN_API int rn_mask_head_create(rn_ctx *ctx, rn_mask_head **out, uint64_t in_channels, uint64_t n_layers,
                               const uint64_t *layer_channels, uint64_t dim_reduced, uint64_t classes, uint64_t resolution);
RN_API int rn_mask_head_set_tensor(rn_mask_head *mh, const char *key, const float *host_data, uint64_t numel);
RN_API int rn_mask_head_finalize(rn_mask_head *mh);
RN_API int rn_mask_head_destroy(rn_mask_head *mh);
RN_API int rn_mask_head_forward(rn_mask_head *mh, const float *pooled_nhwc, const int32_t *labels,
                                const float *boxes /* nullable */, uint64_t K, uint64_t image_h, uint64_t image_w,
                                const rn_mask_request *req);
/* The mask head behind the neck and inside a forward.  rn_fpn_forward_masks: rn_fpn_forward_detections plus the mask head
 * and its request; rn_model_forward_masks(_u8): rn_model_forward_detections(_u8)'s arguments plus them.  One more step
 * behind the box head's ("mask_stage" of layer "roi_heads" in the profile, one record per part).  A part of a launch
 * batch forms the RoIs of its own D = detections_per_img detection rows per image (rn_detection_rois_forward's rule),
 * pools them NHWC (M x M, the request's levels, sampling_ratio, aligned and canonical pair; the scales torchvision's, as
 * the pooler's are formed) from its own slice of the neck's scratch, runs the head and writes its own [b] rows of
 * rois [B*D, 5], pooled [B*D, M, M, a], probs [B, D, 2M, 2M], masks and bits [B, D, H, W] (H x W: the call's image);
 * every row of every non-NULL output is written once per forward, and the values are those of the stand-alone entry
 * points on the same rows, bit for bit.  Refused like the detections' calls, and: a mask head without a box head, a
 * detect request whose boxes or labels is NULL, a mask head whose in_channels is not the neck's out_channels, a request
 * out of range or with probs, masks and bits all NULL, a pooled off a 16-byte boundary, an output of the request sharing
 * a byte with any other output of the call.  Every other forward kind issues exactly the launches it issued. */
RN_API int rn_fpn_forward_masks(rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh, const void *const *x_nhwc,
                                uint64_t B, const uint64_t *h, const uint64_t *w, float *const *out_nchw /* nullable */,
                                uint64_t image_h, uint64_t image_w, const rn_rpn_request *req, const rn_roi_pool *rois,
                                const rn_detect_request *det_req, const rn_mask_request *mask_req);
RN_API int rn_model_forward_masks(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh,
                                  const float *input_nchw, uint64_t B, const rn_model_outputs *outs /* nullable */,
                                  const int *stages, const rn_fpn_outputs *fpn_out /* nullable */, const rn_rpn_request *req,
                                  const rn_roi_pool *rois, const rn_detect_request *det_req, const rn_mask_request *mask_req,
                                  int mode);
RN_API int rn_model_forward_masks_u8(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh,
                                     const uint8_t *input_nhwc, uint64_t B, const rn_model_outputs *outs, const int *stages,
                                     const rn_fpn_outputs *fpn_out, const rn_rpn_request *req, const rn_roi_pool *rois,
                                     const rn_detect_request *det_req, const rn_mask_request *mask_req, int mode);

/* ---- The keypoint head behind the box head: convs, 4x4 deconv, bicubic argmax (rn_keypoint.hip) -------------------------
 * torchvision's keypoint branch of RoIHeads in eval mode: keypoint_roi_pool on the DETECTED boxes, KeypointRCNNHeads (3x3
 * convolutions with bias and ReLU), KeypointRCNNPredictor (kps_score_lowres, a ConvTranspose2d(., Kp, 4, 2, 1), then
 * interpolate(scale_factor=2, mode="bilinear", align_corners=False)), keypointrcnn_inference / heatmaps_to_keypoints.  fp32
 * only, like the box and mask heads.  Every entry point is asynchronous on the context's stream, allocates and uploads
 * nothing at forward time (the object's scratch aside), uses no atomics, and refuses with RN_ERR_INVALID -- nothing
 * launched, rn_last_error names the operand -- a NULL operand, an operand off its boundary, an output sharing a byte with
 * another operand, a size out of range; K == 0 is RN_OK with nothing launched.
 *
 * The transposed convolution is ONE 1x1 panel of 16*Kp channels: with W [Cin, Kp, 4, 4] in torch's layout, the panel's row
 * k*16 + ky*4 + kx is W[:, k, ky, kx], no shift, no ReLU, and its output t [K, M, M, 16*Kp] holds the products only (the
 * 16 taps of one keypoint: 64 contiguous bytes of a pixel).  Kernel 4 at stride 2 overlaps: the overlap-add is the predict
 * launch's.
 *
 * rn_keypoint_predict_forward: t (16-byte aligned), bias [Kp], boxes [K, 4], labels [K] int32 or NULL (all valid), M 1..16,
 * Kp 1..256, max_h and max_w 1..8192 -> heat [K, Kp, S, S] (S = 4M) and / or keypoints [K, Kp, 3] with scores [K, Kp].
 * One launch, one block per (detection, keypoint), which reads its 16 columns of t once and forms both maps in LDS; with
 * heat == NULL no heat map reaches memory.  Not all three outputs may be NULL; keypoints and scores come together; boxes
 * and labels are read only where keypoints is given.
 * rn_heatmaps_to_keypoints_forward: the same search (the same device code, the same bits) on a caller's heat
 * [K, Kp, S, S], S 1..64.
 *
 * The arithmetic is a contract; every fp32 operation is rounded on its own, no product fused into an add
 * (keypoint.heatmaps_ref and keypoint.heatmaps_to_keypoints_ref restate it in numpy; the kernel matches them bit for bit):
 *   low[oy][ox] (2M x 2M) starts at bias[k] and adds the valid taps t[iy][ix][k*16 + ky*4 + kx], 2 iy = oy + 1 - ky and
 *     2 ix = ox + 1 - kx, in ascending ky, then ascending kx: at most 2 x 2 of them.
 *   heat is low resized 2M -> 4M by rn_upsample_bilinear_forward's per-axis rule and sum order (the scale is 0.5).
 *   w = max(x2 - x1, 1.0f), h likewise; Wr = (int)ceilf(w), Hr = (int)ceilf(h).  A row is OUT when a box coordinate is not
 *     finite, when Wr > max_w or Hr > max_h, or when its label is below 1 (where labels is given); it answers (0, 0, 0)
 *     and score 0 for every keypoint.  Nothing a box holds decides how long a launch runs beyond max_h x max_w.
 *   The bicubic resize S -> n_out per axis, output index o:
 *     scale = (float)S / (float)n_out                          (one fp32 division, on the device)
 *     src = fl(fl(scale * fl((float)o + 0.5f)) - 0.5f)          NOT clamped at 0: torch's cubic rule
 *     i = floorf(src), tt = fl(src - i); the taps i-1 .. i+2, each clamped to [0, S-1]
 *     with A = -0.75: c0 = ((A*x - 5A)*x + 8A)*x - 4A at x = tt + 1;  c1 = ((A+2)*x - (A+3))*x*x + 1 at x = tt;
 *                     c2: c1's form at x = 1 - tt;  c3: c0's form at x = 2 - tt
 *     a row value is ((c0*v0 + c1*v1) + c2*v2) + c3*v3 over the columns; the output is the same expression over the four
 *     row values (the kernel computes a row value once per (source row, output column): the same operations).
 *   The argmax over the Hr x Wr values: the lowest flat index y*Wr + x that holds the maximum -- index 0 to start with,
 *     replaced only where v > best, so a NaN never replaces (torch's argmax would pick it: the one stated deviation) and
 *     a NaN at index 0 stays.  The result does not depend on the block's thread count.
 *   x = fl(fl(fl((float)x_int + 0.5f) * fl(w / (float)Wr)) + x1), y likewise; keypoints[k][j] = (x, y, 1.0f),
 *     scores[k][j] = best.
 *
 * The object.  rn_keypoint_head_create(ctx, &kh, in_channels, n_layers (1..8), layer_channels[], keypoints Kp, resolution
 * M (1..16)); channel counts are multiples of 64.  rn_keypoint_head_set_tensor takes host fp32, keys with or without the
 * "roi_heads." prefix: keypoint_head.{0,2,4,..}.weight|bias ([c_i, c_{i-1}, 3, 3], [c_i]) and
 * keypoint_predictor.kps_score_lowres.weight|bias ([c_last, Kp, 4, 4], [Kp]).  rn_keypoint_head_forward: pooled_nhwc
 * [K, M, M, in_channels] fp32 (16-byte aligned), labels [K] or NULL, boxes [K, 4] (NULL: the request wants heat only),
 * the image size (max_h, max_w) and the request -> n_layers + 1 contractions (one launch each, or two where the plan
 * finishes a chunked K sum in a second pass) and ONE predict launch.  Of the request it reads heat, keypoints and scores;
 * the pooler's parameters, rois and pooled are the route's.  The scratch -- two ping-pong maps and t -- grows on demand,
 * never on a stream that is being captured and never while a captured graph of the context lives. */
typedef struct rn_keypoint_request {
    int n_levels, level[4];            /* the keypoint pooler's levels of the neck, as rn_roi_pool's */
    int sampling_ratio, aligned;
    double canonical_scale;            /* 224 */
    int canonical_level;               /* 4 */
    float *rois;                       /* [B*D, 5] or NULL */
    float *pooled;                     /* [B*D, M, M, a] or NULL */
    float *heat;                       /* [B, D, Kp, 4M, 4M] or NULL */
    float *keypoints;                  /* [B, D, Kp, 3] or NULL */
    float *scores;                     /* [B, D, Kp] or NULL */
} rn_keypoint_request;
typedef struct rn_keypoint_head rn_keypoint_head;
RN_API int rn_keypoint_predict_forward(rn_ctx *ctx, const float *t, const float *bias, const float *boxes,
                                       const int32_t *labels /* nullable */, uint64_t K, uint64_t M, uint64_t Kp, uint64_t max_h,
                                       uint64_t max_w, float *heat /* nullable */, float *keypoints /* nullable */,
                                       float *scores /* nullable */);
RN_API int rn_heatmaps_to_keypoints_forward(rn_ctx *ctx, const float *heat, const float *boxes, const int32_t *labels /* nullable */,
                                            uint64_t K, uint64_t Kp, uint64_t S, uint64_t max_h, uint64_t max_w, float *keypoints,
                                            float *scores);
RN_API int rn_keypoint_head_create(rn_ctx *ctx, rn_keypoint_head **out, uint64_t in_channels, uint64_t n_layers,
                                   const uint64_t *layer_channels, uint64_t keypoints, uint64_t resolution);
RN_API int rn_keypoint_head_set_tensor(rn_keypoint_head *kh, const char *key, const float *host_data, uint64_t numel);
RN_API int rn_keypoint_head_finalize(rn_keypoint_head *kh);
RN_API int rn_keypoint_head_destroy(rn_keypoint_head *kh);
RN_API int rn_keypoint_head_forward(rn_keypoint_head *kh, const float *pooled_nhwc, const int32_t *labels /* nullable */,
                                    const float *boxes /* nullable */, uint64_t K, uint64_t image_h, uint64_t image_w,
                                    const rn_keypoint_request *req);
/* The keypoint head behind the neck and inside a forward: rn_fpn_forward_masks' / rn_model_forward_masks(_u8)'s arguments
 * plus the keypoint head and its request; the mask head and its request may be NULL (torchvision allows both heads at
 * once).  One more step behind the mask head's ("keypoint_stage" of layer "roi_heads" in the profile, one record per
 * part).  A part of a launch batch forms the RoIs of its own detection rows, pools them NHWC from its own slice of the
 * neck's scratch, runs the head and writes its own rows of rois [B*D, 5], pooled [B*D, M, M, a], heat [B, D, Kp, 4M, 4M],
 * keypoints [B, D, Kp, 3] and scores [B, D, Kp] once; max_h x max_w is the call's image; the values are those of the
 * stand-alone entry points on the same rows, bit for bit.  Refused like the masks' calls, and: a keypoint head without a
 * box head, a detect request whose boxes or labels is NULL, a keypoint head whose in_channels is not the neck's
 * out_channels, a request that wants nothing, an image over 8192 a side, an output of the request sharing a byte with any
 * other output of the call.  Every other forward kind issues exactly the launches it issued. */
RN_API int rn_fpn_forward_keypoints(rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh /* nullable */,
                                    rn_keypoint_head *kh, const void *const *x_nhwc, uint64_t B, const uint64_t *h,
                                    const uint64_t *w, float *const *out_nchw /* nullable */, uint64_t image_h, uint64_t image_w,
                                    const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req,
                                    const rn_mask_request *mask_req /* nullable */, const rn_keypoint_request *kp_req);
RN_API int rn_model_forward_keypoints(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh /* nullable */,
                                      rn_keypoint_head *kh, const float *input_nchw, uint64_t B,
                                      const rn_model_outputs *outs /* nullable */, const int *stages,
                                      const rn_fpn_outputs *fpn_out /* nullable */, const rn_rpn_request *req,
                                      const rn_roi_pool *rois, const rn_detect_request *det_req,
                                      const rn_mask_request *mask_req /* nullable */, const rn_keypoint_request *kp_req, int mode);
RN_API int rn_model_forward_keypoints_u8(rn_model *m, rn_fpn *fpn, rn_rpn *rpn, rn_box_head *bh, rn_mask_head *mh /* nullable */,
                                         rn_keypoint_head *kh, const uint8_t *input_nhwc, uint64_t B,
                                         const rn_model_outputs *outs, const int *stages, const rn_fpn_outputs *fpn_out,
                                         const rn_rpn_request *req, const rn_roi_pool *rois, const rn_detect_request *det_req,
                                         const rn_mask_request *mask_req /* nullable */, const rn_keypoint_request *kp_req,
                                         int mode);
/* Run one forward, then time every tile candidate of every convolution at batch B on the
 * device (events on the context's stream, on the buffers that forward used) and remember the fastest per layer for
 * that batch size.  Results do not change (candidates are bit-identical), only speed. */
RN_API int rn_model_tune(rn_model *m, const float *input_nchw, uint64_t B, float *logits, int mode);
/* The table that rn_model_tune filled, as 64-bit words (header: architecture, element type, fusion
 * settings, batch, mode, candidate count of the build; then the (tile, launch batch) slots of every
 * layer), and its way into another model of the same architecture / element type / settings on an
 * identical device (and of the same input size, rn_model_set_input_size): the shards of a node take over ONE shard's measurement (rn_shard_tune), a later
 * process a stored one.  export with words == NULL returns the size in *n_words; import refuses a
 * table measured for anything else (RN_ERR_INVALID, nothing changed).  Tiles change speed only. */
RN_API int rn_model_export_tuning(const rn_model *m, uint64_t *words, uint64_t cap, uint64_t *n_words);
RN_API int rn_model_import_tuning(rn_model *m, const uint64_t *words, uint64_t n_words);
/* per-op timing of the next forwards: 1 = bracket every op with events */
/* Fused mode only: run conv3 + downsample of the first block of each stage as one contraction
 * (rn_conv2d_nhwc_pair_forward_dt); on by default, off = downsample first, then conv3 with it
 * as the residual.  Changing it invalidates the tuned tiles.  NOT bit-neutral: the pair has one
 * epilogue, so both batch-norm scales are folded into the weight rows (rounded once more) instead of
 * multiplying the fp32 sums; both forms are within the fused mode's tolerance of the reference. */
RN_API int rn_model_set_pair_fusion(rn_model *m, int on);
/* fp32 models: stem through rn_conv2d_nhwc_exact_forward (K = 160; default) or through the
 * 4-channel / 8-slot form of rn_conv2d_nhwc_forward (K = 224).  Invalidates the tuned tiles. */
RN_API int rn_model_set_stem_exact(rn_model *m, int on);
/* streams = 1, 2 or 4: a (sub-)batch runs as that many contiguous parts (of at least 64 images
 * each) on streams of their own -- the launches of one part fill the tails of the others';
 * every image's logits are independent of what else is in its launch, so no bit changes.
 * Default: 2 (measured at B = 256: fp32 +0.8 %, bf16 storage +5..9 %: its 256-wide tiles leave
 * CUs idle in the late stages); as long as this function has not been called, an fp32 model splits
 * only into parts of at least 128 images (parts of 96 measured 3 % slower than one stream, parts
 * of 64 equal).  Profiled and tuning forwards always use one stream.  Tuned tiles
 * are kept per launch batch size (rn_model_tune times the parts' size and the whole batch), so
 * switching between the tuned part count and one stream keeps them.  streams = 0 returns to the
 * library default (as if this function had never been called). */
RN_API int rn_model_set_streams(rn_model *m, int streams);
RN_API int rn_model_get_streams(const rn_model *m);
/* the number of parts (streams) a forward of B images actually runs as under the rule above */
RN_API int rn_model_parts(const rn_model *m, uint64_t B);
/* parts = 1 (default), 2, 4, 8 or 16: the stem, the max-pool and the first stage -- the layers
 * with the largest tensors -- run in that many slices of each batch part, one after the other,
 * so that what one kernel writes is still in the 256 MB Infinity Cache when the next reads it;
 * the other stages then run on the whole part.  Same bits.  Invalidates the tuned tiles. */
RN_API int rn_model_set_front_parts(rn_model *m, int parts);
RN_API int rn_model_set_profiling(rn_model *m, int on);
/* after a profiled forward + rn_sync: number of ops, then one record per op */
RN_API uint64_t rn_model_profile_count(const rn_model *m);
RN_API int rn_model_profile_get(const rn_model *m, uint64_t index, const char **op_name,
                                const char **layer_name, float *ms, double *flops,
                                double *bytes);
RN_API uint64_t rn_model_activation_bytes(const rn_model *m);

/* ---- exact-K small-Cin form (fp32): the 7x7x3 stem as K = 147 -> 160 -----------------
 * rn_conv2d_nhwc_forward pads a 3-channel image to 4 channels and 8 kernel-column slots
 * (K = 7*32 = 224 per output for 147 real products).  This form reads a physically padded
 * [B,Hp,Wp,Cin] image (rn_nchw_to_nhwc_pad_dt with Cpad = Cin and border = the convolution's
 * padding; Hp = H + 2*pad) with dword gathers and packs K = k*k*Cin contiguously, rounded up
 * to a multiple of 32 — 5 K tiles instead of 7 for the ResNet stem (conv1, main.cu:111). */
RN_API uint64_t rn_conv2d_packed_weight_numel_exact(uint64_t in_channels, uint64_t out_channels,
                                                    uint64_t kernel_size);
RN_API int rn_conv2d_pack_weight_exact(rn_ctx *ctx, const float *weight_oihw, float *packed,
                                       uint64_t in_channels, uint64_t out_channels,
                                       uint64_t kernel_size);
RN_API int rn_conv2d_nhwc_exact_forward(rn_ctx *ctx, const float *inp_padded, float *out,
                                        const float *packed_exact_weight, uint64_t kernel_size,
                                        uint64_t stride, uint64_t h_out, uint64_t w_out,
                                        uint64_t B, uint64_t in_channels, uint64_t out_channels,
                                        uint64_t Hp, uint64_t Wp, const rn_epilogue *epilogue);

/* ---- fused stem: conv 7x7/2 + folded batch-norm + ReLU + max-pool 3x3/2/1 in one launch ----
 * The first four ops of the reference's forward (main.cu:179-192) without ever writing the
 * 112x112x64 stem tensor: a direct convolution out of an LDS-resident input patch, the pool as
 * LDS integer maxima of the non-negative ReLU outputs.  inp_padded: NHWC image that carries its
 * own 3-pixel zero border (rn_nchw_to_nhwc_pad_dt with border 3; Cpad = 3 for fp32, 4 for
 * bf16), [B,Hp,Wp,Cpad]; out: [B,PH,PW,64] of `dtype`.  Needs 64 output channels, a conv
 * output width that is a multiple of 8 and at most 128 (ResNet: 112), any height; bf16: an even
 * Wp.  A block walks down an image (or a segment of it, rn_ctx_set_stem_items) and carries the
 * pooled row two consecutive row groups share in LDS.  scale/shift: per channel, nullable.  Same products as conv + bn + relu + maxpool, summed in another order.
 * relu must be non-zero (RN_ERR_INVALID otherwise): the pool is taken as an integer maximum of
 * the non-negative ReLU outputs' bit patterns. */
RN_API uint64_t rn_stem_pool_packed_weight_numel(int dtype);
RN_API int rn_stem_pool_pack_weight_dt(rn_ctx *ctx, int dtype, const float *weight_oihw /* [64,Cin,7,7] */,
                                       void *packed, uint64_t in_channels);
RN_API int rn_stem_pool_forward_dt(rn_ctx *ctx, int dtype, const void *inp_padded, void *out,
                                   const void *packed_weight, const float *scale, const float *shift,
                                   int relu, uint64_t B, uint64_t Hp, uint64_t Wp);
/* The same launch reading the reference's fp32 NCHW image [B,in_channels,H,W] directly: the zero
 * border, the channel interleave and the conversion to `dtype` happen while the input patch is
 * assembled in LDS, so no layout kernel and no padded copy of the image are needed.  W % 4 == 0. */
RN_API int rn_stem_pool_nchw_forward_dt(rn_ctx *ctx, int dtype, const float *inp_nchw, void *out,
                                        const void *packed_weight, const float *scale,
                                        const float *shift, int relu, uint64_t B,
                                        uint64_t in_channels, uint64_t H, uint64_t W);
/* The same launch for a caller that names the stem tensor as an output of its own (the reference does:
 * main.cu:179-190 keeps conv -> bn -> relu in `act1`, then pools it): stem_out [B,Ho,Wo,64] = relu(bn(conv(x))),
 * NHWC fp32, written from the registers that feed the pool, beside pool_out [B,PH,PW,64].  fp32, NCHW image
 * [B,in_channels,H,W], W % 4 == 0; otherwise as rn_stem_pool_nchw_forward_dt.  What the deferred route
 * (rn_ctx_set_deferred) runs for conv 7x7/2 -> bn -> relu -> maxpool 3x3/2/1. */
RN_API int rn_stem_conv_pool_nchw_forward(rn_ctx *ctx, const float *inp_nchw, float *stem_out, float *pool_out,
                                          const void *packed_weight, const float *scale, const float *shift,
                                          uint64_t B, uint64_t in_channels, uint64_t H, uint64_t W);
/* conv3 + bn3 + residual add + ReLU of one bottleneck block and conv1 + bn1 + ReLU of the next
 * (layerForward, main.cu:131-164, end of one pass and start of the next) as ONE launch on bf16 or
 * fp32 NHWC tensors: t2 [rows][mid] -> y [rows][channels] (written: the next block's residual) ->
 * t1 [rows][next_mid]; y reaches conv1 through LDS instead of HBM.  The same bits as the two
 * separate rn_conv2d_nhwc_forward_dt calls.  (mid, channels, next_mid) = (64, 256, 64 | 128) or, bf16
 * only, (128, 512, 128); packed weights from rn_conv2d_pack_weight_dt; scale/shift may be NULL. */
RN_API int rn_conv_chain_forward_dt(rn_ctx *ctx, int dtype, const void *t2, const void *residual,
                                    void *y, const void *packed_w3, const float *scale3,
                                    const float *shift3, void *t1, const void *packed_w1,
                                    const float *scale1, const float *shift1, uint64_t rows,
                                    uint64_t mid_channels, uint64_t channels, uint64_t next_mid);
/* The same chain out of the fused conv3 + downsample pair of a stage's first block
 * (rn_conv2d_nhwc_pair_forward_dt: panel from rn_conv2d_pack_weight_pair_dt with the scales folded
 * in, K = mid + in2 channels, no residual): y = relu(t2 . w3s + x2 . wds + shift), then conv1.
 * in2_channels 64; fp32: next_mid 64. */
RN_API int rn_conv_chain_pair_forward_dt(rn_ctx *ctx, int dtype, const void *t2, const void *x2,
                                         void *y, const void *packed_pair, const float *shift,
                                         void *t1, const void *packed_w1, const float *scale1,
                                         const float *shift1, uint64_t rows, uint64_t mid_channels,
                                         uint64_t in2_channels, uint64_t channels, uint64_t next_mid);
/* Fused mode: conv3 of a block and conv1 of the block after it as one launch where a chain kernel
 * exists (rn_conv_chain_forward_dt; default on).  The same bits whatever the setting. */
RN_API int rn_model_set_chain(rn_model *m, int on);
/* Fused mode: use it for conv1 + bn1 + relu + maxpool (default on; fp32 needs the exact-K stem
 * image, rn_model_set_stem_exact).  on == 2: through rn_stem_pool_nchw_forward_dt, the input
 * layout launch disappears as well.  Invalidates the tuned tiles.  on = 1 and on = 2 give the same
 * bits; on = 0 (stem and max-pool as separate launches) sums the 147 products of an output in another
 * order (another K padding), so its results differ in the last bits -- which is why the model keeps
 * ONE setting for every batch size. */
RN_API int rn_model_set_stem_pool_fusion(rn_model *m, int on);

/* ---- fused pair: out = epilogue(conv(inp, W1) + conv1x1(inp2, W2)) ------------------
 * One contraction whose K loop runs through both convolutions: the bottleneck's conv3 and the
 * block's downsample convolution (main.cu:134-147) without writing and re-reading the
 * downsample tensor.  One accumulator, so each branch's BatchNorm scale is folded into its
 * weight rows when the pair is packed; the epilogue then carries only the summed shifts
 * (scale = NULL), an optional residual and ReLU.  The second convolution is 1x1 / padding 0
 * and must produce the same [B,h_out,w_out,Cout] shape.  Both channel counts must be
 * multiples of 32 (fp32) / 64 (bf16): RN_ERR_UNSUPPORTED otherwise. */
typedef struct rn_conv_second {
    const void *inp;      /* [B,H,W,in_channels] NHWC, element type = dtype */
    uint64_t in_channels, H, W, stride;
} rn_conv_second;
RN_API uint64_t rn_conv2d_packed_pair_weight_numel(uint64_t in_channels, uint64_t out_channels,
                                                   uint64_t kernel_size, uint64_t in_channels2);
/* rows [Cout][k*k*Cin + Cin2]; scale1 / scale2 (per out channel, nullable = 1) multiply the rows */
RN_API int rn_conv2d_pack_weight_pair_dt(rn_ctx *ctx, int dtype, const float *w1_oihw,
                                         const float *scale1, const float *w2_oihw,
                                         const float *scale2, void *packed, uint64_t in_channels,
                                         uint64_t out_channels, uint64_t kernel_size,
                                         uint64_t in_channels2);
RN_API int rn_conv2d_nhwc_pair_forward_dt(rn_ctx *ctx, int dtype, int out_dtype, const void *inp,
                                          void *out, const void *packed_pair_weight,
                                          uint64_t kernel_size, uint64_t stride, uint64_t padding,
                                          uint64_t h_out, uint64_t w_out, uint64_t B,
                                          uint64_t in_channels, uint64_t out_channels, uint64_t H,
                                          uint64_t W, const rn_conv_second *second,
                                          const rn_epilogue *epilogue);

/* ---- captured forward ---------------------------------------------------------------
 * The forward of one (input, B, logits, mode) as a hipGraph: ~57 launches (RN-50, fused) replayed
 * by one call.  Worth it at small B, where the launches' host cost is comparable to their GPU
 * time; at B=256 the GPU is the bound either way.  Capture runs one eager forward first (arenas
 * and scratch are allocated outside the capture) and bakes in the tile choice of that moment
 * (call rn_model_tune before).  Needs profiling and sync_each_op off (RN_ERR_INVALID otherwise).
 * The buffers must stay valid while the graph lives; while any graph of a context lives, a
 * call that would have to grow the context's scratch or the model's activation arenas (a
 * larger batch than any before) returns RN_ERR_INVALID instead of moving them.
 * Teardown order: rn_graph_destroy, then rn_model_destroy, then rn_ctx_destroy.  A graph points into
 * its model's arenas and into the scratch of the contexts the model owns for its extra streams:
 * rn_model_destroy returns RN_ERR_INVALID (and frees nothing) while a graph captured from the model
 * lives. */
typedef struct rn_graph rn_graph;
RN_API int rn_model_capture(rn_model *m, const float *input_nchw, uint64_t B, float *logits,
                            int mode, rn_graph **out);
RN_API int rn_graph_launch(rn_graph *g); /* asynchronous, on the context's stream */
RN_API int rn_graph_destroy(rn_graph *g);
RN_API uint64_t rn_graph_node_count(const rn_graph *g);

/* ---- host pipeline: overlapped upload / forward / download --------------------------
 * What main() of the reference does once (H2D of the image, forward, D2H of the logits:
 * main.cu:236-240) as a stream of batches: two slots; the upload of batch i+1 (pinned
 * staging -> device, on a copy stream) runs beside the forward of batch i.  submit() blocks
 * only when both slots are busy; collect() returns the logits of the oldest batch. */
typedef struct rn_pipeline rn_pipeline;
RN_API int rn_pipeline_create(rn_model *m, rn_pipeline **out, uint64_t B, int mode);
RN_API int rn_pipeline_destroy(rn_pipeline *p);
/* The pinned staging buffer (B*3*H*W floats, the model's input size when the pipeline was created -- it
 * cannot change while the pipeline lives) the next submit will upload from: a decoder
 * that writes its output there saves the host-side copy.  RN_ERR_INVALID when both slots are
 * busy. */
RN_API int rn_pipeline_input_buffer(rn_pipeline *p, float **host_staging);
/* host_input_nchw: B*3*H*W floats in any host memory (copied into the staging buffer), or
 * NULL / the pointer rn_pipeline_input_buffer returned when the staging buffer is already
 * filled. */
RN_API int rn_pipeline_submit(rn_pipeline *p, const float *host_input_nchw);
/* host_logits: B*classes floats (rn_model_classes of the model when the pipeline was created).
 * RN_ERR_INVALID when nothing is in flight. */
RN_API int rn_pipeline_collect(rn_pipeline *p, float *host_logits);
RN_API uint64_t rn_pipeline_in_flight(const rn_pipeline *p);
/* The same for a batch of n <= B images (a ragged last batch), and with the class indices
 * (first maximum wins, main.cu:243-249) next to the logits; host_logits ([n,classes]), host_top1
 * ([n]) and n may each be NULL. */
RN_API int rn_pipeline_submit_n(rn_pipeline *p, const float *host_input_nchw, uint64_t n);
RN_API int rn_pipeline_collect_n(rn_pipeline *p, float *host_logits, uint64_t *host_top1, uint64_t *n);
/* A pipeline for 8-bit RGB input ([n,H,W,3], rn_model_forward_u8): pinned staging and device
 * input buffers of B*H*W*3 bytes (B*150528 at 224 x 224), a quarter of the fp32 pipeline's upload and staging copy.
 * Collect as above.  A pipeline takes the input format it was created for: the float calls on a
 * byte pipeline, and these on a float pipeline, return RN_ERR_INVALID. */
RN_API int rn_pipeline_create_u8(rn_model *m, rn_pipeline **out, uint64_t B, int mode);
RN_API int rn_pipeline_input_buffer_u8(rn_pipeline *p, uint8_t **host_staging);
/* host_input_nhwc: n*H*W*3 bytes in any host memory, or NULL / the staging pointer; n <= B */
RN_API int rn_pipeline_submit_u8_n(rn_pipeline *p, const uint8_t *host_input_nhwc, uint64_t n);
/* A pipeline for decoded images of any size (rn_model_forward_images_u8): pinned staging and device
 * input buffers hold the packed batch -- at most max_batch_bytes of pixels -- and behind it the
 * coefficient tables, uploaded together on the copy stream.  host_imgs: n <= B pointers to the images
 * in any host memory (image i: heights[i] x widths[i] x 3 bytes); they are packed back to back into
 * staging.  Collect as above.  A batch of more than max_batch_bytes, or the call on a pipeline of
 * another input format (and the float / byte calls on this one), is RN_ERR_INVALID.  A model whose
 * input size is not 224 x 224: RN_ERR_UNSUPPORTED at creation. */
RN_API int rn_pipeline_create_images_u8(rn_model *m, rn_pipeline **out, uint64_t B, int mode,
                                        uint64_t max_batch_bytes);
RN_API int rn_pipeline_submit_images_u8_n(rn_pipeline *p, const uint8_t *const *host_imgs,
                                          const uint64_t *heights, const uint64_t *widths, uint64_t n);

/* ---- one batch over several devices of a node ---------------------------------------
 * The multi-device form of the reference's main() (main.cu:228-254).  The forward has no
 * cross-image reduction, so the batch shards contiguously (shard g of G owns images
 * [lo, hi) of rn_shard_bounds), weights are replicated, no data moves between devices and the
 * logits are concatenated on the host.  One host thread + one context + one model per listed
 * device, created and driven by the group; a device may be listed more than once.  Calls on a
 * group are serialised by the caller.  host_* pointers are host memory; host_logits
 * ([B,1000]) and host_top1 ([B], first maximum wins as main.cu:243-249) may each be NULL. */
typedef struct rn_shard rn_shard;
RN_API void rn_shard_bounds(uint64_t B, int rank, int world, uint64_t *lo, uint64_t *hi);
RN_API int rn_shard_create(rn_shard **out, const int *devices, int n_devices, int arch);
/* the same group over models of rn_model_create_ex(depth, groups, width_per_group) */
RN_API int rn_shard_create_ex(rn_shard **out, const int *devices, int n_devices, int depth, int groups,
                              int width_per_group);
RN_API int rn_shard_destroy(rn_shard *g);
RN_API int rn_shard_count(const rn_shard *g);
RN_API const char *rn_shard_last_error(const rn_shard *g);
RN_API int rn_shard_set_tensor(rn_shard *g, const char *key, const float *host_data, uint64_t numel);
RN_API int rn_shard_load_dir(rn_shard *g, const char *weights_dir);
RN_API int rn_shard_set_dtype(rn_shard *g, int dtype);
RN_API int rn_shard_finalize(rn_shard *g);
RN_API int rn_shard_forward(rn_shard *g, const float *host_input_nchw, uint64_t B,
                            float *host_logits, uint64_t *host_top1, int mode);
/* Tuned tiles for the launches the group will issue for batches of B: with a stream open
 * (rn_shard_stream_open) those of a whole shard per device, otherwise those of rn_shard_forward's
 * chunks (at most 128 images).  ONE shard measures (rn_model_tune on shard 0, the other devices
 * idle), the shards with the same share take its table over (rn_model_import_tuning: identical
 * devices, and every shard then runs the same tiles); a shard with another share (uneven split)
 * measures for itself.  Refused while submitted batches are in flight. */
RN_API int rn_shard_tune(rn_shard *g, const float *host_input_nchw, uint64_t B, int mode);
/* Where shard `rank` runs: its device, the NUMA node of that device and the CPUs its host thread was
 * bound to ("" = not bound).  A shard's thread is bound to the cores local to its device
 * (rn_device_locality, intersected with the cores the process may use) when it starts: it copies every
 * batch from the caller's pageable memory into pinned staging, and on a two-socket node the remote
 * socket's memory path halves that copy.  Best effort; RN_SHARD_AFFINITY=0 in the environment turns it off. */
RN_API int rn_shard_placement(const rn_shard *g, int rank, int *device, int *numa_node, char *cpulist,
                              uint64_t cpulist_cap);
/* Shard `rank`'s model, for settings and queries (rn_model_set_streams, rn_model_export_tuning ...)
 * between calls on the group, when its host thread is parked.  Owned by the group; running a forward
 * on it from the caller's thread is not supported (its context belongs to the shard's thread). */
RN_API rn_model *rn_shard_model(rn_shard *g, int rank);
/* Upload, forward and download overlap on every device (main.cu:236-240 and tensor.cuh:184-199
 * do them strictly in sequence, from pageable memory): each device owns an rn_pipeline -- pinned
 * staging, a copy stream, two slots.  rn_shard_forward sends a shard through it in chunks of at
 * most 128 images, two in flight.  The streaming form below keeps two whole BATCHES in flight:
 *   rn_shard_stream_open(g, B, mode);            shard r owns images rn_shard_bounds(B, r, G)
 *   rn_shard_submit(g, batch0); rn_shard_submit(g, batch1);
 *   rn_shard_collect(g, logits0, top1_0); rn_shard_submit(g, batch2); ...
 * submit returns once every device has queued its shard (the copy into pinned staging is done
 * by the device's own host thread, all devices in parallel); collect returns the oldest batch,
 * rows in image order.  rn_shard_stream_buffer gives shard `rank`'s pinned staging buffer of the
 * NEXT submit and the image range [lo, hi) it holds: a decoder that writes there and submits
 * NULL saves the host-side copy.  At most two batches in flight (RN_ERR_INVALID otherwise).
 * rn_shard_forward re-sizes the per-device pipelines for its own chunks: it is refused while
 * submitted batches are in flight, and a stream must be opened again after it. */
RN_API int rn_shard_stream_open(rn_shard *g, uint64_t B, int mode);
RN_API int rn_shard_stream_buffer(rn_shard *g, int rank, float **host_staging, uint64_t *lo,
                                  uint64_t *hi);
RN_API int rn_shard_submit(rn_shard *g, const float *host_input_nchw /* NULL: staging filled */);
RN_API int rn_shard_collect(rn_shard *g, float *host_logits, uint64_t *host_top1);
RN_API int rn_shard_in_flight(const rn_shard *g);
/* The same from 8-bit RGB input ([B,224,224,3] host bytes; same contiguous split, shard r's images
 * start r's lo * 150528 bytes in): one call, or a stream opened for bytes, whose staging buffers a
 * decoder fills directly.  collect, in_flight and close are those above; the float submit / buffer
 * calls on a byte stream, and the reverse, return RN_ERR_INVALID. */
RN_API int rn_shard_forward_u8(rn_shard *g, const uint8_t *host_input_nhwc, uint64_t B,
                               float *host_logits, uint64_t *host_top1, int mode);
RN_API int rn_shard_stream_open_u8(rn_shard *g, uint64_t B, int mode);
RN_API int rn_shard_stream_buffer_u8(rn_shard *g, int rank, uint8_t **host_staging, uint64_t *lo,
                                     uint64_t *hi);
RN_API int rn_shard_submit_u8(rn_shard *g, const uint8_t *host_input_nhwc /* NULL: staging filled */);
RN_API int rn_shard_stream_close(rn_shard *g);

#ifdef __cplusplus
}
#endif
#endif /* RN_HIP_H */
