/* rn_params.h -- the named parameters of an object (a neck, a head) as a table it declares at create time, and the
 * host copies that set_tensor leaves in it until finalize.  Pure host code (plain C, no context, no device):
 * rn_stage.hip wraps it into refusals and uploads. */
#ifndef RN_PARAMS_H
#define RN_PARAMS_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { RN_PARAMS_MAX = 44, RN_PARAM_KEY = 64 };

/* A tensor of the state dict, `rows` rows of `len` values, and the shape it is stored in on the device: `prows` rows
 * of `pitch`, every added element `fill` (most objects store what they are given: prows = rows, pitch = len). */
typedef struct rn_params_entry {
    char key[RN_PARAM_KEY], alt[RN_PARAM_KEY]; /* alt: another spelling of the key, or "" */
    uint64_t rows, len, prows, pitch;
    float fill;
    float *host; /* the caller's rows * len values, or NULL: not set */
} rn_params_entry;

typedef struct rn_params {
    int n;
    const char *prefix; /* accepted in front of every key ("roi_heads."), or NULL */
    rn_params_entry p[RN_PARAMS_MAX];
} rn_params;

/* returns the entry's index, or -1 when the table is full or a key does not fit (nothing is written then) */
static inline int rn_params_add(rn_params *t, const char *key, const char *alt, uint64_t rows, uint64_t len, uint64_t prows,
                                uint64_t pitch, float fill)
{
    rn_params_entry *e;
    if (t->n >= RN_PARAMS_MAX || strlen(key) >= RN_PARAM_KEY || (alt && strlen(alt) >= RN_PARAM_KEY)) return -1;
    e = &t->p[t->n];
    memset(e, 0, sizeof(*e));
    strcpy(e->key, key);
    if (alt) strcpy(e->alt, alt);
    e->rows = rows, e->len = len, e->prows = prows, e->pitch = pitch, e->fill = fill;
    return t->n++;
}

/* the entry `key` names in either spelling, with or without the table's prefix, or -1 */
static inline int rn_params_find(const rn_params *t, const char *key)
{
    int i;
    const size_t np = t->prefix ? strlen(t->prefix) : 0;
    if (np && strncmp(key, t->prefix, np) == 0) key += np;
    for (i = 0; i < t->n; ++i)
        if (strcmp(key, t->p[i].key) == 0 || (t->p[i].alt[0] && strcmp(key, t->p[i].alt) == 0)) return i;
    return -1;
}

/* Keeps a copy of data as entry i.  *wanted: the entry's element count, rows * len.  Returns 0, 1 when numel is not
 * that count, 2 when the host is out of memory.  A second set overwrites the first copy. */
static inline int rn_params_set(rn_params *t, int i, const float *data, uint64_t numel, uint64_t *wanted)
{
    rn_params_entry *e = &t->p[i];
    *wanted = e->rows * e->len;
    if (numel != *wanted) return 1;
    if (!e->host) e->host = (float *)malloc(numel * sizeof(float));
    if (!e->host) return 2;
    memcpy(e->host, data, numel * sizeof(float));
    return 0;
}

/* the first entry that is not set, or -1 */
static inline int rn_params_first_missing(const rn_params *t)
{
    int i;
    for (i = 0; i < t->n; ++i)
        if (!t->p[i].host) return i;
    return -1;
}

/* entry i as it is stored: dst [prows, pitch], the entry's rows at the front of its first rows, `fill` elsewhere */
static inline void rn_params_write(const rn_params *t, int i, float *dst)
{
    const rn_params_entry *e = &t->p[i];
    uint64_t r, j;
    for (j = 0; j < e->prows * e->pitch; ++j) dst[j] = e->fill;
    for (r = 0; r < e->rows; ++r) memcpy(dst + r * e->pitch, e->host + r * e->len, e->len * sizeof(float));
}

static inline void rn_params_free(rn_params *t)
{
    int i;
    for (i = 0; i < t->n; ++i) free(t->p[i].host), t->p[i].host = NULL;
}

#endif /* RN_PARAMS_H */
