// The operand lists of rn_operands.h on their own: pure host code over addresses, so this program needs neither the
// library nor a device.  It feeds the three questions overlapping, adjacent, absent and empty operands and exits 0
// when every answer is the expected one.  Meant to be built with the host sanitizers:
// (the runtimes linked into the program, so that nothing has to be preloaded):
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -Iresnet.c_amd/csrc examples/operands_check.cpp
#include <cstdio>
#include <cstdlib>

#include "rn_operands.h"

static int failures = 0;

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) ++failures, std::printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

int main()
{
    // one real allocation: the addresses are the data, nothing is read or written through them
    char *mem = static_cast<char *>(std::malloc(4096));
    if (!mem) return 2;
    const char *p = mem + (16 - reinterpret_cast<uintptr_t>(mem) % 16) % 16;
    int with = -7;

    // alignment: 4 bytes for everything but arrays of bytes; absent operands are never asked
    {
        const rn_operand ok[] = {{p, 64, "a", 1, 0}, {p + 65, 7, "bytes", 1, 1}, {nullptr, 64, "absent", 1, 0}, {p + 128, 0, "empty", 0, 0}};
        EXPECT(rn_operands_misaligned(ok, 4) == -1);
        const rn_operand off[] = {{p, 64, "a", 1, 0}, {p + 66, 8, "b", 0, 0}};
        EXPECT(rn_operands_misaligned(off, 2) == 1);
        EXPECT(rn_operands_misaligned(off, 0) == -1);
    }
    // inside one list: adjacent is fine, one shared byte is not, two inputs may share, an absent one shares nothing
    {
        const rn_operand adjacent[] = {{p, 64, "out", 1, 0}, {p + 64, 64, "in", 0, 0}, {p + 128, 64, "out2", 1, 0}};
        EXPECT(rn_operands_clash(adjacent, 3, &with) == -1);
        const rn_operand one_byte[] = {{p, 65, "out", 1, 0}, {p + 64, 64, "in", 0, 0}};
        EXPECT(rn_operands_clash(one_byte, 2, &with) == 0 && with == 1);
        const rn_operand inputs[] = {{p, 64, "in", 0, 0}, {p + 8, 64, "in2", 0, 0}};
        EXPECT(rn_operands_clash(inputs, 2, &with) == -1);
        const rn_operand absent[] = {{nullptr, ~0ull, "absent", 1, 0}, {p, 64, "in", 0, 0}, {p + 8, 8, "late", 1, 0}};
        EXPECT(rn_operands_clash(absent, 3, &with) == 2 && with == 1);
        const rn_operand inside[] = {{p + 16, 4, "small", 0, 0}, {p, 64, "out", 1, 0}};
        EXPECT(rn_operands_clash(inside, 2, &with) == 1 && with == 0);
        const rn_operand same[] = {{p, 64, "out", 1, 0}, {p, 64, "out2", 1, 0}};
        EXPECT(rn_operands_clash(same, 2, &with) == 0 && with == 1);
    }
    // between groups: what a call of the neck's tail builds, in small
    {
        const rn_operand maps[] = {{p, 256, "x[0]", 0, 0}, {p + 256, 128, "x[1]", 0, 0}};
        const rn_operand levels[] = {{p + 512, 256, "level[0]", 1, 0}, {nullptr, 256, "level[1]", 1, 0}};
        rn_operand roi[] = {{p + 1024, 128, "pooled", 1, 0}, {nullptr, 32, "levels_out", 1, 0}, {p + 1280, 160, "rois_dev", 0, 0}};
        rn_operand rpn[] = {{p + 1536, 128, "out.boxes", 1, 0}, {p + 1792, 160, "out.rois", 1, 0}, {p + 2048, 33, "cand.valid", 1, 1}};
        const rn_operand_group g[4] = {{maps, 2}, {levels, 2}, {roi, 3}, {rpn, 3}};
        const rn_operand *a = nullptr, *b = nullptr;
        EXPECT(!rn_operand_groups_clash(g, 4, &a, &b));
        EXPECT(!rn_operand_groups_clash(g, 0, &a, &b) && !rn_operand_groups_clash(g, 1, &a, &b));
        roi[0].ptr = p + 252;  // pooled over the last bytes of an input map, and on into the next
        EXPECT(rn_operand_groups_clash(g, 4, &a, &b) && a == &roi[0] && b == &maps[0]);
        roi[0].ptr = p + 384;  // adjacent to the second map: its first byte is that map's first free one
        EXPECT(!rn_operand_groups_clash(g, 4, &a, &b));
        roi[2].ptr = p + 4;  // an input over an input: no one's business
        EXPECT(!rn_operand_groups_clash(g, 4, &a, &b));
        roi[2].ptr = p + 516;  // an input over an exported level
        EXPECT(rn_operand_groups_clash(g, 4, &a, &b) && a == &roi[2] && b == &levels[0]);
        roi[2].ptr = rpn[1].ptr;  // rois_dev on the rpn's out.rois: refused ...
        EXPECT(rn_operand_groups_clash(g, 4, &a, &b) && a == &rpn[1] && b == &roi[2]);
        roi[2].ptr = nullptr;  // ... unless the chain takes it out of the list: out.rois stands for it
        EXPECT(!rn_operand_groups_clash(g, 4, &a, &b));
        rpn[2].ptr = p + 1024 + 127;  // an array of bytes on the last byte of pooled
        roi[0].ptr = p + 1024;
        EXPECT(rn_operand_groups_clash(g, 4, &a, &b) && a == &rpn[2] && b == &roi[0]);
        roi[0].bytes = 0;  // a pooler of no RoIs is in nobody's way, wherever its pointers are
        EXPECT(!rn_operand_groups_clash(g, 4, &a, &b));
    }
    // the sixth group: a mask head's request behind a box head's, its pasted outputs the largest buffers of the call
    {
        const rn_operand maps[] = {{p, 64, "x[0]", 0, 0}};
        const rn_operand levels[] = {{nullptr, 64, "level[0]", 1, 0}};
        const rn_operand roi[] = {{p + 64, 64, "pooled", 1, 0}, {nullptr, 8, "levels_out", 1, 0}, {nullptr, 40, "rois_dev", 0, 0}};
        const rn_operand rpn[] = {{p + 128, 32, "out.boxes", 1, 0}, {p + 160, 40, "out.rois", 1, 0}};
        rn_operand box[] = {{p + 256, 64, "out.boxes", 1, 0}, {p + 320, 16, "out.labels", 1, 0}, {nullptr, 16, "out.scores", 1, 0}};
        rn_operand mask[] = {{p + 512, 80, "mask.rois", 1, 0}, {nullptr, 256, "mask.pooled", 1, 0}, {p + 768, 256, "mask.probs", 1, 0},
                             {p + 1024, 1024, "mask.masks", 1, 0}, {p + 2048, 256, "mask.bits", 1, 1}};
        const rn_operand_group g[6] = {{maps, 1}, {levels, 1}, {roi, 3}, {rpn, 2}, {box, 3}, {mask, 5}};
        const rn_operand *a = nullptr, *b = nullptr;
        EXPECT(rn_operands_misaligned(mask, 5) == -1 && rn_operands_clash(mask, 5, &with) == -1);
        EXPECT(!rn_operand_groups_clash(g, 6, &a, &b));
        mask[4].ptr = p + 2047;  // the bytes one byte into the fp32 masks: the stage's own list answers
        EXPECT(rn_operands_clash(mask, 5, &with) == 3 && with == 4);
        mask[4].ptr = p + 2049;  // arrays of bytes sit anywhere
        EXPECT(rn_operands_misaligned(mask, 5) == -1 && rn_operands_clash(mask, 5, &with) == -1);
        mask[3].ptr = p + 1026;
        EXPECT(rn_operands_misaligned(mask, 5) == 3);
        mask[3].ptr = p + 1024;
        mask[2].ptr = box[0].ptr;  // the probabilities on the detections the stage reads
        EXPECT(rn_operand_groups_clash(g, 6, &a, &b) && a == &mask[2] && b == &box[0]);
        mask[2].ptr = p + 768;
        mask[0].ptr = p + 335;  // the RoI rows over the last byte of the labels
        EXPECT(rn_operand_groups_clash(g, 6, &a, &b) && a == &mask[0] && b == &box[1]);
        mask[0].ptr = p + 336;  // adjacent
        EXPECT(!rn_operand_groups_clash(g, 6, &a, &b));
        mask[3].ptr = p;  // the pasted masks over an input map of the family
        EXPECT(rn_operand_groups_clash(g, 6, &a, &b) && a == &mask[3] && b == &maps[0]);
        mask[3].ptr = nullptr;  // not wanted: in nobody's way
        EXPECT(!rn_operand_groups_clash(g, 6, &a, &b));
        box[2].ptr = p + 800;  // an output of the box head inside the probabilities
        EXPECT(rn_operand_groups_clash(g, 6, &a, &b) && a == &mask[2] && b == &box[2]);
    }
    // the seventh group: a keypoint head's request behind the mask head's (or without one: an empty sixth group)
    {
        const rn_operand maps[] = {{p, 64, "x[0]", 0, 0}};
        const rn_operand levels[] = {{nullptr, 64, "level[0]", 1, 0}};
        const rn_operand roi[] = {{p + 64, 64, "pooled", 1, 0}, {nullptr, 8, "levels_out", 1, 0}, {nullptr, 40, "rois_dev", 0, 0}};
        const rn_operand rpn[] = {{p + 128, 32, "out.boxes", 1, 0}, {p + 160, 40, "out.rois", 1, 0}};
        const rn_operand box[] = {{p + 256, 64, "out.boxes", 1, 0}, {p + 320, 16, "out.labels", 1, 0}, {nullptr, 16, "out.scores", 1, 0}};
        rn_operand mask[] = {{p + 512, 80, "mask.rois", 1, 0}, {nullptr, 256, "mask.pooled", 1, 0}, {p + 768, 256, "mask.probs", 1, 0},
                             {p + 1024, 1024, "mask.masks", 1, 0}, {p + 2048, 256, "mask.bits", 1, 1}};
        rn_operand kp[] = {{p + 2304, 80, "keypoint.rois", 1, 0}, {nullptr, 256, "keypoint.pooled", 1, 0},
                           {p + 2560, 768, "keypoint.heat", 1, 0}, {p + 3328, 144, "keypoint.keypoints", 1, 0},
                           {p + 3472, 48, "keypoint.scores", 1, 0}};
        rn_operand_group g[7] = {{maps, 1}, {levels, 1}, {roi, 3}, {rpn, 2}, {box, 3}, {mask, 5}, {kp, 5}};
        const rn_operand *a = nullptr, *b = nullptr;
        EXPECT(rn_operands_misaligned(kp, 5) == -1 && rn_operands_clash(kp, 5, &with) == -1);
        EXPECT(!rn_operand_groups_clash(g, 7, &a, &b));
        kp[4].ptr = p + 3468;  // the scores over the last keypoint: the stage's own list answers
        EXPECT(rn_operands_clash(kp, 5, &with) == 3 && with == 4);
        kp[4].ptr = p + 3474;
        EXPECT(rn_operands_misaligned(kp, 5) == 4);
        kp[4].ptr = p + 3472;
        kp[2].ptr = p + 2300;  // the heat maps over the last byte of the mask's bits
        EXPECT(rn_operand_groups_clash(g, 7, &a, &b) && a == &kp[2] && b == &mask[4]);
        kp[2].ptr = p + 2560;
        kp[3].ptr = box[0].ptr;  // the keypoints on the detections the stage reads
        EXPECT(rn_operand_groups_clash(g, 7, &a, &b) && a == &kp[3] && b == &box[0]);
        kp[3].ptr = p + 3328;
        kp[0].ptr = p + 335;  // the RoI rows over the last byte of the labels
        EXPECT(rn_operand_groups_clash(g, 7, &a, &b) && a == &kp[0] && b == &box[1]);
        kp[0].ptr = mask[0].ptr;  // the two heads' RoI rows are two outputs: they may not be one buffer
        EXPECT(rn_operand_groups_clash(g, 7, &a, &b) && a == &kp[0] && b == &mask[0]);
        g[5].n = 0;  // no mask head: its request is in nobody's way
        EXPECT(!rn_operand_groups_clash(g, 7, &a, &b));
        g[5].n = 5;
        kp[0].ptr = p + 2304;
        kp[2].ptr = nullptr;  // not wanted: in nobody's way
        mask[3].ptr = p + 2600;
        mask[3].bytes = 64;
        EXPECT(!rn_operand_groups_clash(g, 7, &a, &b));
        kp[3].ptr = p;  // the keypoints over an input map of the family
        EXPECT(rn_operand_groups_clash(g, 7, &a, &b) && a == &kp[3] && b == &maps[0]);
    }
    std::free(mem);
    std::printf(failures ? "%d expectations failed\n" : "operands_check: every expectation holds\n", failures);
    return failures ? 1 : 0;
}
