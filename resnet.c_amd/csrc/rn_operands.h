/* rn_operands.h -- the buffers of a call as a list, and the two questions every entry point asks of such lists.
 * Pure host code over addresses (plain C, no context, no device): rn_internal.h wraps it into refusals. */
#ifndef RN_OPERANDS_H
#define RN_OPERANDS_H

#include <stddef.h>
#include <stdint.h>

typedef struct rn_operand {
    const void *ptr; /* NULL: absent, never in anyone's way */
    uint64_t bytes;  /* 0: nothing is read or written */
    const char *name;
    int output;     /* the call writes it */
    int bytes_only; /* an array of bytes: any boundary */
} rn_operand;

static inline int rn_operand_shares(const rn_operand *a, const rn_operand *b)
{
    const uintptr_t x = (uintptr_t)a->ptr, y = (uintptr_t)b->ptr;
    return a->ptr && b->ptr && x < y + b->bytes && y < x + a->bytes;
}

/* the first operand that is off a 4-byte boundary (arrays of bytes: any), or -1 */
static inline int rn_operands_misaligned(const rn_operand *ops, int n_ops)
{
    int i;
    for (i = 0; i < n_ops; ++i)
        if (ops[i].ptr && !ops[i].bytes_only && ((uintptr_t)ops[i].ptr & 3) != 0) return i;
    return -1;
}

/* inside one list: the first output that shares a byte with another operand (*with: that one), or -1 */
static inline int rn_operands_clash(const rn_operand *ops, int n_ops, int *with)
{
    int i, j;
    for (i = 0; i < n_ops; ++i) {
        if (!ops[i].output) continue;
        for (j = 0; j < n_ops; ++j) {
            if (j == i || (ops[j].output && j < i)) continue;
            if (rn_operand_shares(&ops[i], &ops[j])) return *with = j, i;
        }
    }
    return -1;
}

/* A call's operands in groups (one per stage, one for the entry family's own): inside a group its own check_operands
 * has spoken; between groups no output may share a byte with any operand of another group.  Returns 1 and the first
 * such pair (*a of the later group, *b of the earlier one), or 0.  Two inputs may share what they like, and an
 * operand of no bytes (a pooler of no RoIs) is in nobody's way. */
typedef struct rn_operand_group {
    const rn_operand *ops;
    int n;
} rn_operand_group;

static inline int rn_operand_groups_clash(const rn_operand_group *g, int n_groups, const rn_operand **a, const rn_operand **b)
{
    int gi, gj, i, j;
    for (gi = 1; gi < n_groups; ++gi)
        for (gj = 0; gj < gi; ++gj)
            for (i = 0; i < g[gi].n; ++i)
                for (j = 0; j < g[gj].n; ++j) {
                    const rn_operand *x = &g[gi].ops[i], *y = &g[gj].ops[j];
                    if ((x->output || y->output) && x->bytes && y->bytes && rn_operand_shares(x, y)) return *a = x, *b = y, 1;
                }
    return 0;
}

#endif /* RN_OPERANDS_H */
