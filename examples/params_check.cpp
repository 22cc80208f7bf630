// The parameter table of rn_params.h on its own: pure host code, so this program needs neither the library nor a
// device.  It declares the tables of a 2-level neck, an RPN, a box head and a 2-layer mask head the way their create
// functions do, asks for every key in every spelling, sets, overwrites and writes out, and exits 0 when every answer
// is the expected one.  Meant to be built with the host sanitizers (the runtimes linked into the program, so that
// nothing has to be preloaded; the leak check at exit is part of the test):
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -Iresnet.c_amd/csrc examples/params_check.cpp
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rn_params.h"

static int failures = 0;

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) ++failures, std::printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

static int add(rn_params *t, const std::string &key, const char *alt, uint64_t rows, uint64_t len)
{
    return rn_params_add(t, key.c_str(), alt, rows, len, rows, len, 0.0f);
}

// rn_fpn_create: level l owns entries 4 l .. 4 l + 3
static void neck(rn_params *t, int levels, const uint64_t *cin, uint64_t a)
{
    for (int l = 0; l < levels; ++l)
        for (int e = 0; e < 4; ++e) {
            const std::string block = e < 2 ? "inner_blocks." : "layer_blocks.", part = e % 2 ? "bias" : "weight";
            const std::string alt = block + std::to_string(l) + "." + part;
            add(t, block + std::to_string(l) + ".0." + part, alt.c_str(), e % 2 ? 1 : a, e == 0 ? cin[l] : e == 2 ? a * 9 : a);
        }
}

// rn_rpn_create
static void rpn(rn_params *t, uint64_t C, uint64_t A)
{
    add(t, "head.conv.0.0.weight", "head.conv.weight", C, C * 9);
    add(t, "head.conv.0.0.bias", "head.conv.bias", 1, C);
    add(t, "head.cls_logits.weight", nullptr, A, C);
    add(t, "head.cls_logits.bias", nullptr, 1, A);
    add(t, "head.bbox_pred.weight", nullptr, 4 * A, C);
    add(t, "head.bbox_pred.bias", nullptr, 1, 4 * A);
}

// rn_box_head_create
static void box_head(rn_params *t, uint64_t F, uint64_t M, uint64_t C)
{
    const char *layer[4] = {"box_head.fc6", "box_head.fc7", "box_predictor.cls_score", "box_predictor.bbox_pred"};
    const uint64_t rows[4] = {M, M, C, 4 * C};
    for (int i = 0; i < 4; ++i) {
        add(t, std::string(layer[i]) + ".weight", nullptr, rows[i], i == 0 ? F : M);
        add(t, std::string(layer[i]) + ".bias", nullptr, 1, rows[i]);
    }
}

// rn_mask_head_create: layer i owns 2 i and 2 i + 1, then conv5_mask and mask_fcn_logits
static void mask_head(rn_params *t, uint64_t Cin, int layers, const uint64_t *ch, uint64_t Cr, uint64_t C)
{
    t->prefix = "roi_heads.";
    for (int i = 0; i < layers; ++i)
        for (int j = 0; j < 2; ++j) {
            const std::string part = j ? "bias" : "weight", alt = "mask_head.mask_fcn" + std::to_string(i + 1) + "." + part;
            add(t, "mask_head." + std::to_string(i) + ".0." + part, alt.c_str(), j ? 1 : ch[i], j ? ch[i] : (i ? ch[i - 1] : Cin) * 9);
        }
    add(t, "mask_predictor.conv5_mask.weight", nullptr, ch[layers - 1], Cr * 4);
    add(t, "mask_predictor.conv5_mask.bias", nullptr, 1, Cr);
    add(t, "mask_predictor.mask_fcn_logits.weight", nullptr, C, Cr);
    add(t, "mask_predictor.mask_fcn_logits.bias", nullptr, 1, C);
}

int main()
{
    // one table per object on the heap: the sanitizer sees every access past an end
    rn_params *fpn = static_cast<rn_params *>(std::calloc(1, sizeof(rn_params)));
    rn_params *rp = static_cast<rn_params *>(std::calloc(1, sizeof(rn_params)));
    rn_params *bh = static_cast<rn_params *>(std::calloc(1, sizeof(rn_params)));
    rn_params *mh = static_cast<rn_params *>(std::calloc(1, sizeof(rn_params)));
    if (!fpn || !rp || !bh || !mh) return 2;
    const uint64_t cin[2] = {64, 128}, ch[2] = {64, 128};
    neck(fpn, 2, cin, 64), rpn(rp, 64, 3), box_head(bh, 256, 64, 5), mask_head(mh, 64, 2, ch, 64, 5);
    EXPECT(fpn->n == 8 && rp->n == 6 && bh->n == 8 && mh->n == 8);

    // every key and every other spelling, to the slot the objects' code indexes
    {
        const char *block[2] = {"inner_blocks.", "layer_blocks."}, *part[2] = {"weight", "bias"};
        for (int l = 0; l < 2; ++l)
            for (int e = 0; e < 4; ++e) {
                const std::string at = block[e / 2] + std::to_string(l);
                EXPECT(rn_params_find(fpn, (at + ".0." + part[e % 2]).c_str()) == 4 * l + e);
                EXPECT(rn_params_find(fpn, (at + "." + part[e % 2]).c_str()) == 4 * l + e);
            }
        const char *rk[8] = {"head.conv.0.0.weight", "head.conv.0.0.bias", "head.cls_logits.weight", "head.cls_logits.bias",
                             "head.bbox_pred.weight", "head.bbox_pred.bias", "head.conv.weight", "head.conv.bias"};
        for (int i = 0; i < 8; ++i) EXPECT(rn_params_find(rp, rk[i]) == (i < 6 ? i : i - 6));
        const char *bk[8] = {"box_head.fc6.weight", "box_head.fc6.bias", "box_head.fc7.weight", "box_head.fc7.bias",
                             "box_predictor.cls_score.weight", "box_predictor.cls_score.bias",
                             "box_predictor.bbox_pred.weight", "box_predictor.bbox_pred.bias"};
        for (int i = 0; i < 8; ++i) EXPECT(rn_params_find(bh, bk[i]) == i);
        const char *mk[12] = {"mask_head.0.0.weight", "mask_head.0.0.bias", "mask_head.1.0.weight", "mask_head.1.0.bias",
                              "mask_predictor.conv5_mask.weight", "mask_predictor.conv5_mask.bias",
                              "mask_predictor.mask_fcn_logits.weight", "mask_predictor.mask_fcn_logits.bias",
                              "mask_head.mask_fcn1.weight", "mask_head.mask_fcn1.bias", "mask_head.mask_fcn2.weight",
                              "mask_head.mask_fcn2.bias"};
        for (int i = 0; i < 12; ++i) {
            EXPECT(rn_params_find(mh, mk[i]) == (i < 8 ? i : i - 8));
            // the prefix: accepted where the table has one, refused where it has none
            EXPECT(rn_params_find(mh, (std::string("roi_heads.") + mk[i]).c_str()) == (i < 8 ? i : i - 8));
        }
        EXPECT(rn_params_find(bh, "roi_heads.box_head.fc6.weight") == -1);
        EXPECT(rn_params_find(fpn, "roi_heads.inner_blocks.0.0.weight") == -1);
        EXPECT(rn_params_find(mh, "roi_heads.roi_heads.mask_head.0.0.weight") == -1);
    }
    // unknown: a level or a layer the object does not have, a key cut short, the empty key, the prefix alone
    EXPECT(rn_params_find(fpn, "inner_blocks.2.0.weight") == -1 && rn_params_find(fpn, "inner_blocks.2.weight") == -1);
    EXPECT(rn_params_find(mh, "mask_head.2.0.weight") == -1 && rn_params_find(mh, "mask_head.mask_fcn3.weight") == -1);
    EXPECT(rn_params_find(mh, "mask_head.mask_fcn0.weight") == -1);
    EXPECT(rn_params_find(fpn, "") == -1 && rn_params_find(mh, "") == -1 && rn_params_find(mh, "roi_heads.") == -1);
    EXPECT(rn_params_find(fpn, "inner_blocks.0.0.weigh") == -1 && rn_params_find(fpn, "inner_blocks.0.0.weights") == -1);

    // a wrong numel is refused, the wanted count comes back on its own, nothing is kept
    {
        std::vector<float> v(64 * 128, 1.0f);
        uint64_t wanted = 0;
        const int i = rn_params_find(fpn, "inner_blocks.1.0.weight");
        EXPECT(rn_params_set(fpn, i, v.data(), 64 * 128 - 1, &wanted) == 1 && wanted == 64 * 128);
        EXPECT(fpn->p[i].host == nullptr);
        EXPECT(rn_params_first_missing(fpn) == 0);
    }
    // first-missing names the right key; set twice: the second values are the ones written out, nothing leaks
    {
        uint64_t wanted = 0;
        for (int i = 0; i < rp->n; ++i) {
            if (i == 3) continue;
            std::vector<float> v(rp->p[i].rows * rp->p[i].len, 1e3f);
            EXPECT(rn_params_set(rp, i, v.data(), v.size(), &wanted) == 0 && wanted == v.size());
        }
        EXPECT(rn_params_first_missing(rp) == 3 && std::string(rp->p[3].key) == "head.cls_logits.bias");
        std::vector<float> a(3, 1e3f), b = {1.0f, 2.0f, 3.0f}, out(3, -1.0f);
        EXPECT(rn_params_set(rp, 3, a.data(), 3, &wanted) == 0);
        const float *first = rp->p[3].host;
        EXPECT(rn_params_set(rp, 3, b.data(), 3, &wanted) == 0 && rp->p[3].host == first);
        EXPECT(rn_params_first_missing(rp) == -1);
        rn_params_write(rp, 3, out.data());
        EXPECT(out == b);
    }
    // the padded write-out: rows = 3, len = 5 into prows = 4, pitch = 8, every added element the fill
    {
        rn_params *t = static_cast<rn_params *>(std::calloc(1, sizeof(rn_params)));
        if (!t) return 2;
        uint64_t wanted = 0;
        EXPECT(rn_params_add(t, "padded", nullptr, 3, 5, 4, 8, 0.5f) == 0);
        std::vector<float> v(15), out(32, -1.0f);
        for (int i = 0; i < 15; ++i) v[i] = (float)(i + 1);
        EXPECT(rn_params_set(t, 0, v.data(), 32, &wanted) == 1 && wanted == 15);
        EXPECT(rn_params_set(t, 0, v.data(), 15, &wanted) == 0);
        rn_params_write(t, 0, out.data());
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 8; ++c) EXPECT(out[r * 8 + c] == (r < 3 && c < 5 ? (float)(r * 5 + c + 1) : 0.5f));
        // the table at its capacity refuses one more entry (and a key that does not fit) instead of writing past an end
        int last = 0;
        for (int i = 1; i < RN_PARAMS_MAX; ++i) last = rn_params_add(t, ("k" + std::to_string(i)).c_str(), nullptr, 1, 1, 1, 1, 0.0f);
        EXPECT(last == RN_PARAMS_MAX - 1 && t->n == RN_PARAMS_MAX);
        EXPECT(rn_params_add(t, "one more", nullptr, 1, 1, 1, 1, 0.0f) == -1 && t->n == RN_PARAMS_MAX);
        EXPECT(rn_params_find(t, "one more") == -1 && rn_params_find(t, ("k" + std::to_string(RN_PARAMS_MAX - 1)).c_str()) == last);
        EXPECT(rn_params_add(fpn, std::string(RN_PARAM_KEY, 'x').c_str(), nullptr, 1, 1, 1, 1, 0.0f) == -1 && fpn->n == 8);
        EXPECT(rn_params_add(fpn, "short", std::string(RN_PARAM_KEY, 'x').c_str(), 1, 1, 1, 1, 0.0f) == -1 && fpn->n == 8);
        rn_params_free(t);
        EXPECT(t->p[0].host == nullptr);
        std::free(t);
    }
    rn_params_free(fpn), rn_params_free(rp), rn_params_free(bh), rn_params_free(mh);
    rn_params_free(rp);  // a second free finds nothing
    std::free(fpn), std::free(rp), std::free(bh), std::free(mh);
    if (failures) return std::printf("%d expectations failed\n", failures), 1;
    std::printf("every expectation holds\n");
    return 0;
}
