/*
 * rn_infer -- plain-C driver, the main() of the reference (cuda/inference/main.cu:228-254):
 * build the model from weights_bin/, read test_bins/<image>.bin, run the forward pass,
 * print "max index is N" per image.  The reference hard-codes everything (ResNet-152,
 * B = 1, paths); here the same defaults can be overridden from the command line.
 *
 *   rn_infer [--arch 18|34|50|101|152|resnext50_32x4d|resnext101_32x8d|resnext101_64x4d|wide_resnet50_2|wide_resnet101_2] [--weights DIR] [--input FILE | --u8 FILE | --rgb FILE --hw H,W] [--batch B]
 *            [--size H,W] [--dilate a,b,c] [--maps PREFIX] [--segment HEAD_DIR --labels FILE] [--mode fused|ops] [--dtype f32|bf16] [--device N | --devices a,b,c,...]
 *
 * --size H,W sets the model's input size (rn_model_set_input_size; default 224,224; single device only):
 * --input then holds B x 3 x H x W floats and --u8 B x H x W x 3 bytes, and a file of any other length is
 * refused with the size in the message.
 * --dilate a,b,c (each 0 or 1) is torchvision's replace_stride_with_dilation for layer2, layer3, layer4
 * (rn_model_set_dilation; bottleneck networks, single device only): the same weights at output stride 16, 8 or 4.
 * --maps PREFIX also writes the feature maps behind layer1..layer4 of the batch it ran, from the same forward
 * (rn_model_forward_maps): PREFIX.layer1.bin .. PREFIX.layer4.bin, each [B,C,H,W] fp32 (rn_save_f32_file; the
 * shapes are rn_model_stage_shape's).  Single device, not with --rgb; the lines printed are unchanged.
 * --segment HEAD_DIR --labels FILE also writes the label map of the batch it ran, from the same forward
 * (rn_model_forward_segment): HEAD_DIR/<key> holds the seven fp32 tensors of torchvision's FCNHead
 * (classifier.0.weight .. classifier.4.bias; in_channels is the model's feature width, mid_channels a quarter of
 * it, the class count is the length of classifier.4.bias), FILE receives B x H x W label bytes at the model's
 * input size.  Works with --size, --dilate, --dtype and --u8; single device, not with --rgb or --maps; the lines
 * printed are unchanged.
 * --u8 FILE reads B x 150528 raw bytes, the decoder's 8-bit RGB crops ([B,224,224,3]), instead of
 * the preprocessed fp32 file: the device normalises them (rn_model_forward_u8), same lines out.
 * --rgb FILE --hw H,W reads the H x W x 3 raw bytes of ONE decoded image of any size: the device resizes
 * (short side 256, PIL's antialiased bilinear bits) and centre-crops it (rn_model_forward_images_u8) and
 * the line printed is the one --u8 prints on the crop PIL makes.  Single device only.
 * --dtype bf16 stores activations and weights as bf16 (fused mode only).
 *
 * --devices shards the batch contiguously over the listed devices (rn_shard_*: one host
 * thread + context + model per device, no data moves between devices) and prints the class
 * indices in image order, exactly as the single-device run does.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rn_hip.h"

#define CHECK(ctx, expr)                                                                  \
    do {                                                                                  \
        int st_ = (expr);                                                                 \
        if (st_ != RN_OK) {                                                               \
            fprintf(stderr, "rn_infer: %s failed: %s (%s)\n", #expr, rn_status_string(st_), \
                    (ctx) ? rn_last_error(ctx) : "");                                     \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

/* the whole file, which must hold exactly `want` bytes; NULL (and a message) otherwise */
static uint64_t size_h = 224, size_w = 224; /* --size */

static void *read_exact(const char *path, uint64_t want, uint64_t B, int u8)
{
    void *host = malloc(want);
    FILE *f = fopen(path, "rb");
    if (!host || !f || fread(host, 1, want, f) != want || fgetc(f) != EOF) {
        if (u8)
            fprintf(stderr, "rn_infer: %s: %s: --u8 takes %llu x %llu x 3 8-bit RGB images only (--size); the file does not "
                            "hold exactly %llu bytes (batch %llu)\n", rn_status_string(RN_ERR_UNSUPPORTED), path,
                    (unsigned long long)size_h, (unsigned long long)size_w, (unsigned long long)want,
                    (unsigned long long)B);
        else
            fprintf(stderr, "rn_infer: %s: %s: the model driver takes 3 x %llu x %llu fp32 images only (--size); the file "
                            "does not hold exactly %llu floats (batch %llu)\n", rn_status_string(RN_ERR_UNSUPPORTED),
                    path, (unsigned long long)size_h, (unsigned long long)size_w,
                    (unsigned long long)(want / sizeof(float)), (unsigned long long)B);
        if (f) fclose(f);
        free(host);
        return NULL;
    }
    fclose(f);
    return host;
}

/* HEAD_DIR/key: raw fp32, the weights_bin format; the malloc'd values and their count, NULL when unreadable */
static float *read_f32(const char *dir, const char *key, uint64_t *numel)
{
    char path[1024];
    FILE *f;
    long bytes;
    float *host = NULL;
    snprintf(path, sizeof(path), "%s/%s", dir, key);
    f = fopen(path, "rb");
    if (f && fseek(f, 0, SEEK_END) == 0 && (bytes = ftell(f)) > 0 && bytes % 4 == 0 && fseek(f, 0, SEEK_SET) == 0 &&
        (host = (float *)malloc((size_t)bytes)) != NULL && fread(host, 1, (size_t)bytes, f) == (size_t)bytes) {
        *numel = (uint64_t)bytes / 4;
    } else {
        fprintf(stderr, "rn_infer: %s: %s: cannot read fp32 values\n", rn_status_string(RN_ERR_IO), path);
        free(host);
        host = NULL;
    }
    if (f) fclose(f);
    return host;
}

/* --arch: a ResNet depth, or one of torchvision's ResNeXt / Wide ResNet names */
static int groups_g = 0, wpg_g = 0; /* 0, 0: rn_model_create(arch) */
static int parse_arch(const char *v)
{
    static const struct { const char *name; int depth, groups, wpg; } fam[] = {
        {"resnext50_32x4d", 50, 32, 4}, {"resnext101_32x8d", 101, 32, 8}, {"resnext101_64x4d", 101, 64, 4},
        {"wide_resnet50_2", 50, 1, 128}, {"wide_resnet101_2", 101, 1, 128}};
    unsigned i;
    for (i = 0; i < sizeof(fam) / sizeof(fam[0]); ++i)
        if (!strcmp(v, fam[i].name)) {
            groups_g = fam[i].groups;
            wpg_g = fam[i].wpg;
            return fam[i].depth;
        }
    groups_g = wpg_g = 0;
    return atoi(!strncmp(v, "resnet", 6) ? v + 6 : v);
}

static int run_sharded(const int *devices, int ndev, int arch, const char *weights,
                       const char *input, int u8, uint64_t B, int mode, int dtype)
{
    rn_shard *g = NULL;
    void *host = NULL;
    uint64_t *idx = NULL, b;
    const uint64_t want = B * 3 * 224 * 224 * (u8 ? 1 : sizeof(float));
    int st;
    st = groups_g ? rn_shard_create_ex(&g, devices, ndev, arch, groups_g, wpg_g) : rn_shard_create(&g, devices, ndev, arch);
    if (st != RN_OK) { fprintf(stderr, "rn_infer: rn_shard_create: %s\n", rn_status_string(st)); return 1; }
#define SCHECK(expr)                                                                         \
    do {                                                                                     \
        int st_ = (expr);                                                                    \
        if (st_ != RN_OK) {                                                                  \
            fprintf(stderr, "rn_infer: %s failed: %s (%s)\n", #expr, rn_status_string(st_),  \
                    rn_shard_last_error(g));                                                 \
            return 1;                                                                        \
        }                                                                                    \
    } while (0)
    SCHECK(rn_shard_load_dir(g, weights));
    if (dtype != RN_DTYPE_F32) SCHECK(rn_shard_set_dtype(g, dtype));
    SCHECK(rn_shard_finalize(g));
    printf("created model\n");
    {   /* where every shard's host thread runs (stderr: stdout stays what the single-device run prints) */
        int r;
        for (r = 0; r < rn_shard_count(g); ++r) {
            int dev = -1, node = -1;
            char cpus[256];
            if (rn_shard_placement(g, r, &dev, &node, cpus, sizeof(cpus)) == RN_OK)
                fprintf(stderr, "rn_infer: shard %d on device %d, NUMA node %d, host thread on cpus [%s]\n", r, dev, node,
                        cpus[0] ? cpus : "not bound");
        }
    }
    idx = (uint64_t *)malloc(B * sizeof(uint64_t));
    host = read_exact(input, want, B, u8);
    if (!host || !idx) return 1;
    if (u8)
        SCHECK(rn_shard_forward_u8(g, (const uint8_t *)host, B, NULL, idx, mode));
    else
        SCHECK(rn_shard_forward(g, (const float *)host, B, NULL, idx, mode));
#undef SCHECK
    printf("Finished\n");
    for (b = 0; b < B; ++b) printf("max index is %llu\n", (unsigned long long)idx[b]);
    free(idx);
    free(host);
    rn_shard_destroy(g);
    return 0;
}

int main(int argc, char **argv)
{
    int arch = 152, device = 0, mode = RN_FWD_FUSED, dtype = RN_DTYPE_F32, u8 = 0, i;
    int devices[64], ndev = 0;
    uint64_t B = 1, numel = 0, b, rgb_h = 0, rgb_w = 0, classes = 0, topk = 0, j;
    float *top_prob_dev = NULL, *top_prob = NULL;
    uint64_t *top_idx_dev = NULL, *top_idx = NULL;
    int rgb = 0;
    int dilate[3] = {0, 0, 0}; /* --dilate */
    const char *weights = "weights_bin";
    const char *input = "test_bins/ILSVRC2012_val_00004749.bin";
    const char *maps_prefix = NULL; /* --maps */
    const char *seg_dir = NULL, *labels_path = NULL; /* --segment, --labels */
    rn_seg_head *head = NULL;
    uint8_t *labels_dev = NULL;
    rn_model_maps maps = {{NULL, NULL, NULL, NULL}};
    rn_ctx *ctx = NULL;
    rn_model *model = NULL;
    float *inp = NULL, *logits = NULL;
    uint8_t *inp_u8 = NULL;
    uint64_t *idx_dev = NULL, *idx = NULL;

    for (i = 1; i < argc; ++i) {
        const char *a = argv[i];
        const char *v = (i + 1 < argc) ? argv[i + 1] : NULL;
        if (!strcmp(a, "--arch") && v) { arch = parse_arch(v); ++i; }
        else if (!strcmp(a, "--weights") && v) { weights = v; ++i; }
        else if (!strcmp(a, "--input") && v) { input = v; u8 = 0; ++i; }
        else if (!strcmp(a, "--u8") && v) { input = v; u8 = 1; ++i; }
        else if (!strcmp(a, "--rgb") && v) { input = v; rgb = 1; ++i; }
        else if (!strcmp(a, "--hw") && v) {
            char *q = NULL;
            rgb_h = strtoull(v, &q, 10);
            rgb_w = (q && *q == ',') ? strtoull(q + 1, NULL, 10) : 0;
            ++i;
        }
        else if (!strcmp(a, "--dtype") && v && (!strcmp(v, "f32") || !strcmp(v, "bf16"))) {
            dtype = strcmp(v, "bf16") ? RN_DTYPE_F32 : RN_DTYPE_BF16;
            ++i;
        }
        else if (!strcmp(a, "--size") && v) {
            char *q = NULL;
            size_h = strtoull(v, &q, 10);
            size_w = (q && *q == ',') ? strtoull(q + 1, NULL, 10) : 0;
            ++i;
        }
        else if (!strcmp(a, "--dilate") && v) {
            if (sscanf(v, "%d,%d,%d", &dilate[0], &dilate[1], &dilate[2]) != 3) dilate[0] = -1; /* refused below */
            ++i;
        }
        else if (!strcmp(a, "--maps") && v) { maps_prefix = v; ++i; }
        else if (!strcmp(a, "--segment") && v) { seg_dir = v; ++i; }
        else if (!strcmp(a, "--labels") && v) { labels_path = v; ++i; }
        else if (!strcmp(a, "--batch") && v) { B = strtoull(v, NULL, 10); ++i; }
        else if (!strcmp(a, "--classes") && v) { classes = strtoull(v, NULL, 10); ++i; }
        else if (!strcmp(a, "--topk") && v) { topk = strtoull(v, NULL, 10); ++i; }
        else if (!strcmp(a, "--device") && v) { device = atoi(v); ++i; }
        else if (!strcmp(a, "--devices") && v) {
            const char *q = v;
            while (*q && ndev < 64) {
                devices[ndev++] = (int)strtol(q, (char **)&q, 10);
                if (*q == ',') ++q;
            }
            ++i;
        }
        else if (!strcmp(a, "--mode") && v) { mode = strcmp(v, "ops") ? RN_FWD_FUSED : RN_FWD_REFERENCE_OPS; ++i; }
        else {
            fprintf(stderr, "usage: %s [--arch 18|34|50|101|152|resnext50_32x4d|resnext101_32x8d|resnext101_64x4d|wide_resnet50_2|wide_resnet101_2] [--weights DIR] [--input FILE | --u8 FILE | --rgb FILE --hw H,W] "
                            "[--batch B] [--size H,W] [--dilate a,b,c] [--maps PREFIX] [--segment HEAD_DIR --labels FILE] [--mode fused|ops] [--dtype f32|bf16] [--device N | --devices a,b,...] [--classes N] [--topk K]\n",
                    argv[0]);
            return 2;
        }
    }
    printf("Started\n");
    if (rgb && (ndev > 0 || B != 1 || rgb_h == 0 || rgb_w == 0 || rgb_h > 16384 || rgb_w > 16384)) {
        fprintf(stderr, "rn_infer: %s: --rgb takes one decoded image on one device and needs --hw H,W (sides 1..16384)\n",
                rn_status_string(RN_ERR_UNSUPPORTED));
        return 1;
    }
    if (ndev > 0 && (classes || topk)) {
        fprintf(stderr, "rn_infer: %s: --classes and --topk run on one device (--devices keeps 1000 classes)\n",
                rn_status_string(RN_ERR_UNSUPPORTED));
        return 1;
    }
    if ((size_h != 224 || size_w != 224) && (ndev > 0 || rgb)) {
        fprintf(stderr, "rn_infer: %s: --size other than 224,224 runs on one device and not with --rgb (decoded images are "
                        "cropped to 224 x 224)\n", rn_status_string(RN_ERR_UNSUPPORTED));
        return 1;
    }
    if ((dilate[0] || dilate[1] || dilate[2]) && ndev > 0) {
        fprintf(stderr, "rn_infer: %s: --dilate runs on one device (the shards stay undilated)\n",
                rn_status_string(RN_ERR_UNSUPPORTED));
        return 1;
    }
    if (maps_prefix && (ndev > 0 || rgb)) {
        fprintf(stderr, "rn_infer: %s: --maps runs on one device and not with --rgb\n", rn_status_string(RN_ERR_UNSUPPORTED));
        return 1;
    }
    if ((seg_dir != NULL) != (labels_path != NULL) || (seg_dir && (ndev > 0 || rgb || maps_prefix))) {
        fprintf(stderr, "rn_infer: %s: --segment HEAD_DIR and --labels FILE go together, on one device and not with --rgb "
                        "or --maps\n", rn_status_string(RN_ERR_UNSUPPORTED));
        return 1;
    }
    if (ndev > 0) return run_sharded(devices, ndev, arch, weights, input, u8, B, mode, dtype);
    CHECK(ctx, rn_ctx_create(&ctx, device, NULL));
    CHECK(ctx, groups_g ? rn_model_create_ex(ctx, &model, arch, groups_g, wpg_g) : rn_model_create(ctx, &model, arch));
    if (classes) CHECK(ctx, rn_model_set_classes(model, classes)); /* before the weights: fc.* take its size */
    classes = rn_model_classes(model);
    if (rn_model_set_input_size(model, size_h, size_w) != RN_OK) {
        fprintf(stderr, "rn_infer: %s: --size %llu,%llu: each side must be 32..2048\n", rn_status_string(RN_ERR_INVALID),
                (unsigned long long)size_h, (unsigned long long)size_w);
        return 1;
    }
    if (dilate[0] || dilate[1] || dilate[2]) {
        const int st = rn_model_set_dilation(model, dilate[0], dilate[1], dilate[2]);
        if (st != RN_OK) {
            fprintf(stderr, "rn_infer: %s: --dilate %d,%d,%d: three flags 0 or 1, on a bottleneck network (%s)\n",
                    rn_status_string(st), dilate[0], dilate[1], dilate[2], rn_last_error(ctx));
            return 1;
        }
    }
    CHECK(ctx, rn_model_load_dir(model, weights));
    if (dtype != RN_DTYPE_F32) CHECK(ctx, rn_model_set_dtype(model, dtype));
    CHECK(ctx, rn_model_finalize(model));
    printf("created model\n");

    if (rgb) {
        const uint64_t want = rgb_h * rgb_w * 3;
        void *host = malloc(want);
        FILE *f = fopen(input, "rb");
        if (!host || !f || fread(host, 1, want, f) != want || fgetc(f) != EOF) {
            fprintf(stderr, "rn_infer: %s: %s: --rgb with --hw %llu,%llu takes exactly %llu bytes of 8-bit RGB\n",
                    rn_status_string(RN_ERR_UNSUPPORTED), input, (unsigned long long)rgb_h, (unsigned long long)rgb_w,
                    (unsigned long long)want);
            return 1;
        }
        fclose(f);
        CHECK(ctx, rn_malloc(ctx, (void **)&inp_u8, want));
        CHECK(ctx, rn_memcpy_h2d(ctx, inp_u8, host, want));
        free(host);
    } else if (u8) {
        void *host = read_exact(input, B * size_h * size_w * 3, B, 1);
        if (!host) return 1;
        CHECK(ctx, rn_malloc(ctx, (void **)&inp_u8, B * size_h * size_w * 3));
        CHECK(ctx, rn_memcpy_h2d(ctx, inp_u8, host, B * size_h * size_w * 3));
        free(host);
    } else {
        CHECK(ctx, rn_load_f32_file(ctx, input, &inp, &numel));
    }
    if (!u8 && !rgb && numel != B * 3 * size_h * size_w) {
        fprintf(stderr, "rn_infer: %s: the model driver takes 3 x %llu x %llu fp32 images only (--size); %s holds "
                        "%llu floats, expected %llu for batch %llu\n", rn_status_string(RN_ERR_UNSUPPORTED),
                (unsigned long long)size_h, (unsigned long long)size_w, input,
                (unsigned long long)numel, (unsigned long long)(B * 3 * size_h * size_w),
                (unsigned long long)B);
        return 1;
    }
    CHECK(ctx, rn_malloc(ctx, (void **)&logits, B * classes * sizeof(float)));
    CHECK(ctx, rn_malloc(ctx, (void **)&idx_dev, B * sizeof(uint64_t)));
    if (rgb) {
        const uint64_t zero = 0;
        CHECK(ctx, rn_model_forward_images_u8(model, inp_u8, &zero, &rgb_h, &rgb_w, 1, logits, mode));
    } else if (maps_prefix) { /* the same forward, and the four stage maps out of it */
        rn_model_outputs outs;
        int s;
        memset(&outs, 0, sizeof(outs));
        outs.logits = logits;
        for (s = 0; s < 4; ++s) {
            uint64_t C = 0, H = 0, W = 0;
            CHECK(ctx, rn_model_stage_shape(model, s + 1, &C, &H, &W));
            CHECK(ctx, rn_malloc(ctx, (void **)&maps.layer[s], B * C * H * W * sizeof(float)));
        }
        if (u8)
            CHECK(ctx, rn_model_forward_maps_u8(model, inp_u8, B, &outs, &maps, mode));
        else
            CHECK(ctx, rn_model_forward_maps(model, inp, B, &outs, &maps, mode));
        for (s = 0; s < 4; ++s) {
            uint64_t C = 0, H = 0, W = 0;
            char path[1024];
            CHECK(ctx, rn_model_stage_shape(model, s + 1, &C, &H, &W));
            snprintf(path, sizeof(path), "%s.layer%d.bin", maps_prefix, s + 1);
            CHECK(ctx, rn_save_f32_file(ctx, path, maps.layer[s], B * C * H * W));
        }
    } else if (seg_dir) { /* the same forward, and the label map out of it */
        static const char *const keys[7] = {"classifier.0.weight", "classifier.1.weight", "classifier.1.bias",
                                            "classifier.1.running_mean", "classifier.1.running_var",
                                            "classifier.4.weight", "classifier.4.bias"};
        const uint64_t feat = rn_model_features(model), pixels = B * size_h * size_w;
        uint64_t n = 0;
        rn_model_outputs outs;
        rn_seg_outputs seg;
        uint8_t *host_labels = (uint8_t *)malloc(pixels);
        FILE *f;
        int k;
        float *t = read_f32(seg_dir, keys[6], &n); /* the bias first: its length is the class count */
        if (!t || !host_labels) return 1;
        CHECK(ctx, rn_seg_head_create(ctx, &head, feat, feat / 4, n));
        CHECK(ctx, rn_seg_head_set_dtype(head, dtype));
        CHECK(ctx, rn_seg_head_set_tensor(head, keys[6], t, n));
        free(t);
        for (k = 0; k < 6; ++k) {
            if (!(t = read_f32(seg_dir, keys[k], &n))) return 1;
            CHECK(ctx, rn_seg_head_set_tensor(head, keys[k], t, n));
            free(t);
        }
        CHECK(ctx, rn_seg_head_finalize(head));
        CHECK(ctx, rn_malloc(ctx, (void **)&labels_dev, pixels));
        memset(&outs, 0, sizeof(outs));
        outs.logits = logits;
        seg.labels = labels_dev;
        seg.scores = NULL;
        if (u8)
            CHECK(ctx, rn_model_forward_segment_u8(model, head, inp_u8, B, &outs, &seg, mode));
        else
            CHECK(ctx, rn_model_forward_segment(model, head, inp, B, &outs, &seg, mode));
        CHECK(ctx, rn_memcpy_d2h(ctx, host_labels, labels_dev, pixels));
        f = fopen(labels_path, "wb");
        if (!f || fwrite(host_labels, 1, pixels, f) != pixels || fclose(f) != 0) {
            fprintf(stderr, "rn_infer: %s: %s: cannot write %llu label bytes\n", rn_status_string(RN_ERR_IO), labels_path,
                    (unsigned long long)pixels);
            return 1;
        }
        free(host_labels);
    } else if (u8)
        CHECK(ctx, rn_model_forward_u8(model, inp_u8, B, logits, mode));
    else
        CHECK(ctx, rn_model_forward(model, inp, B, logits, mode));
    CHECK(ctx, rn_argmax_forward(ctx, logits, idx_dev, B, classes));
    idx = (uint64_t *)malloc(B * sizeof(uint64_t));
    if (!idx) return 1;
    CHECK(ctx, rn_memcpy_d2h(ctx, idx, idx_dev, B * sizeof(uint64_t)));
    if (topk) { /* the K best classes by logit with their probabilities, one launch */
        CHECK(ctx, rn_malloc(ctx, (void **)&top_prob_dev, B * topk * sizeof(float)));
        CHECK(ctx, rn_malloc(ctx, (void **)&top_idx_dev, B * topk * sizeof(uint64_t)));
        CHECK(ctx, rn_softmax_topk_forward(ctx, logits, NULL, top_prob_dev, top_idx_dev, B, classes, topk));
        top_prob = (float *)malloc(B * topk * sizeof(float));
        top_idx = (uint64_t *)malloc(B * topk * sizeof(uint64_t));
        if (!top_prob || !top_idx) return 1;
        CHECK(ctx, rn_memcpy_d2h(ctx, top_prob, top_prob_dev, B * topk * sizeof(float)));
        CHECK(ctx, rn_memcpy_d2h(ctx, top_idx, top_idx_dev, B * topk * sizeof(uint64_t)));
    }
    printf("Finished\n");
    for (b = 0; b < B; ++b) {
        printf("max index is %llu\n", (unsigned long long)idx[b]);
        for (j = 0; j < topk; ++j)
            printf("top%llu %llu %.6f\n", (unsigned long long)(j + 1), (unsigned long long)top_idx[b * topk + j],
                   (double)top_prob[b * topk + j]);
    }

    free(idx);
    free(top_prob);
    free(top_idx);
    rn_free(ctx, top_prob_dev);
    rn_free(ctx, top_idx_dev);
    rn_free(ctx, idx_dev);
    rn_free(ctx, logits);
    rn_free(ctx, inp);
    rn_free(ctx, inp_u8);
    for (i = 0; i < 4; ++i) rn_free(ctx, maps.layer[i]);
    rn_free(ctx, labels_dev);
    rn_seg_head_destroy(head);
    rn_model_destroy(model);
    rn_ctx_destroy(ctx);
    return 0;
}
