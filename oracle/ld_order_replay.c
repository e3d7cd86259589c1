/*
 * ld_order_replay.c -- host replay of THE ORDER of the LD product and of the LD scores (TEST INFRASTRUCTURE ONLY).
 *
 * Written from the text of include/viprs_hip.h (sections "LD product" and "LD scores"), not from the kernels:
 *
 *   - the entries of row j lie in a window of W consecutive columns starting at c_lo
 *       symmetric form   c_lo = left_bound[j], W = len_j (the stored window, the diagonal inside it)
 *       upper form       c_lo = the lowest row i < j with i + len_i >= j (j itself if there is none),
 *                        W = j - c_lo + 1 + len_j
 *     (a dense block needs no special case: every row spans the block, so both definitions give the block);
 *   - the entry at column c_lo + e goes to accumulator e % V of lane (e / V) % 64, V = 16 / sizeof(stored LD element); a lane
 *     adds its entries in ascending e, each by ONE fused multiply-add in the state precision T (libm fmaf / fma: a float32
 *     FMA emulated through float64 arithmetic rounds twice); the diagonal and the columns without an entry add an exact
 *     zero, i.e. nothing;
 *   - then a binary tree over the V accumulators of a lane, then the xor butterfly over the 64 lanes.
 *
 * The caller converts the stored LD elements to T (that conversion is one rounding of its own for int32 / int64 / fp64 LD in
 * a float32 state) and applies the epilogues (tests/ld_dot_reference.py `finish`, tests/ld_score_reference.py `finish`).
 * Product: S, the sum before dq_scale.  Scores: S2 with p = fl(x x) and fma(p, a, acc), S0 by plain additions into the same
 * slots; weights == NULL is ONE column of ones.
 *
 * Arrays: left_bound int32 (m), indptr int64 (m + 1), x (indptr[m]) in T, B / weights / outputs (m, n_cols) column-major in T.
 * Return value: 0, or -1 for a bad argument (V not in {2, 4, 8, 16}, a window that leaves 0 .. m - 1).
 * Build: gcc -O2 -std=c11 -ffp-contract=off (no contraction anywhere but the explicit fma).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define LANES 64
#define VMAX 16

/* first[j] of the upper form: rows in ascending order, the first row that reaches j is the lowest */
static int32_t* upper_first(int64_t m, const int64_t* ip) {
    int32_t* first = (int32_t*)malloc(sizeof(int32_t) * (size_t)(m > 0 ? m : 1));
    if (!first) return NULL;
    for (int64_t j = 0; j < m; ++j) first[j] = -1;
    for (int64_t i = 0; i < m; ++i) {
        int64_t hi = i + (ip[i + 1] - ip[i]);
        if (hi > m - 1) hi = m - 1;
        for (int64_t j = hi; j > i && first[j] < 0; --j) first[j] = (int32_t)i;   /* (reached rows are contiguous below hi) */
    }
    for (int64_t j = 0; j < m; ++j)
        if (first[j] < 0) first[j] = (int32_t)j;
    return first;
}

/* the window of row j; returns 0 if it leaves the matrix */
static int row_window(int64_t m, const int32_t* lb, const int64_t* ip, const int32_t* first, int upper, int64_t j,
                      int64_t* c_lo, int64_t* W) {
    const int64_t len = ip[j + 1] - ip[j];
    if (len < 0) return 0;
    if (upper) {
        *c_lo = first[j];
        *W = j - *c_lo + 1 + len;
    } else {
        *c_lo = lb[j];
        *W = len;
    }
    return *c_lo >= 0 && *c_lo + *W <= m;
}

/* position in x of the entry (j, c), c != j, or -1 if the row holds none there */
static int64_t entry_at(const int64_t* ip, int upper, int64_t j, int64_t c_lo, int64_t c) {
    if (!upper) return ip[j] + (c - c_lo);
    if (c > j) return ip[j] + (c - j - 1);
    return c + (ip[c + 1] - ip[c]) >= j ? ip[c] + (j - c - 1) : -1;       /* row c above j: does it reach j? */
}

#define DEFINE_REPLAY(T, SUFFIX, FMA)                                                                                      \
    static T reduce_##SUFFIX(T* acc, int V) {                                                                              \
        for (int l = 0; l < LANES; ++l)                                                                                    \
            for (int w = V / 2; w >= 1; w >>= 1)                                                                           \
                for (int v = 0; v < w; ++v) acc[l * VMAX + v] = acc[l * VMAX + v] + acc[l * VMAX + v + w];                 \
        T t[LANES], u[LANES];                                                                                              \
        for (int l = 0; l < LANES; ++l) t[l] = acc[l * VMAX];                                                              \
        for (int w = 1; w < LANES; w <<= 1) {                                                                              \
            for (int l = 0; l < LANES; ++l) u[l] = t[l] + t[l ^ w];                                                        \
            for (int l = 0; l < LANES; ++l) t[l] = u[l];                                                                   \
        }                                                                                                                  \
        return t[0];                                                                                                       \
    }                                                                                                                      \
                                                                                                                           \
    int ld_replay_dot_##SUFFIX(int64_t m, const int32_t* lb, const int64_t* ip, const T* x, int V, int upper, int n_cols,  \
                               const T* B, T* S) {                                                                         \
        if (m < 0 || n_cols < 1 || (V != 2 && V != 4 && V != 8 && V != 16)) return -1;                                     \
        const int lgV = V == 2 ? 1 : V == 4 ? 2 : V == 8 ? 3 : 4;     /* lane (e / V) % 64, accumulator e % V */           \
        int32_t* first = upper ? upper_first(m, ip) : NULL;                                                                \
        T* acc = (T*)malloc(sizeof(T) * LANES * VMAX * (size_t)n_cols);                                                    \
        int rc = (acc && (first || !upper)) ? 0 : -1;                                                                      \
        for (int64_t j = 0; j < m && rc == 0; ++j) {                                                                       \
            int64_t c_lo, W;                                                                                               \
            if (!row_window(m, lb, ip, first, upper, j, &c_lo, &W)) { rc = -1; break; }                                    \
            for (size_t k = 0; k < (size_t)LANES * VMAX * (size_t)n_cols; ++k) acc[k] = (T)0;                              \
            for (int64_t e = 0; e < W; ++e) {                                                                              \
                const int64_t c = c_lo + e;                                                                                \
                if (c == j) continue;                                                                                      \
                const int64_t at = entry_at(ip, upper, j, c_lo, c);                                                        \
                if (at < 0) continue;                                                                                      \
                const T r = x[at];                                                                                         \
                const size_t slot = (size_t)((e >> lgV) & (LANES - 1)) * VMAX + (size_t)(e & (V - 1));                     \
                for (int g = 0; g < n_cols; ++g) {                                                                         \
                    T* a = acc + (size_t)g * LANES * VMAX + slot;                                                          \
                    *a = FMA(r, B[c + (int64_t)g * m], *a);                                                                \
                }                                                                                                          \
            }                                                                                                              \
            for (int g = 0; g < n_cols; ++g) S[j + (int64_t)g * m] = reduce_##SUFFIX(acc + (size_t)g * LANES * VMAX, V);   \
        }                                                                                                                  \
        free(acc);                                                                                                         \
        free(first);                                                                                                       \
        return rc;                                                                                                         \
    }                                                                                                                      \
                                                                                                                           \
    int ld_replay_scores_##SUFFIX(int64_t m, const int32_t* lb, const int64_t* ip, const T* x, int V, int upper,           \
                                  int n_cols, const T* A, T* S2, T* S0) {                                                  \
        if (m < 0 || n_cols < 1 || (!A && n_cols != 1) || (V != 2 && V != 4 && V != 8 && V != 16)) return -1;              \
        const int lgV = V == 2 ? 1 : V == 4 ? 2 : V == 8 ? 3 : 4;     /* lane (e / V) % 64, accumulator e % V */           \
        int32_t* first = upper ? upper_first(m, ip) : NULL;                                                                \
        T* acc2 = (T*)malloc(sizeof(T) * LANES * VMAX * (size_t)n_cols);                                                   \
        T* acc0 = (T*)malloc(sizeof(T) * LANES * VMAX * (size_t)n_cols);                                                   \
        int rc = (acc2 && acc0 && (first || !upper)) ? 0 : -1;                                                             \
        for (int64_t j = 0; j < m && rc == 0; ++j) {                                                                       \
            int64_t c_lo, W;                                                                                               \
            if (!row_window(m, lb, ip, first, upper, j, &c_lo, &W)) { rc = -1; break; }                                    \
            for (size_t k = 0; k < (size_t)LANES * VMAX * (size_t)n_cols; ++k) acc2[k] = acc0[k] = (T)0;                   \
            for (int64_t e = 0; e < W; ++e) {                                                                              \
                const int64_t c = c_lo + e;                                                                                \
                if (c == j) continue;                                                                                      \
                const int64_t at = entry_at(ip, upper, j, c_lo, c);                                                        \
                if (at < 0) continue;                                                                                      \
                const T r = x[at];                                                                                         \
                const T p = r * r;                                                                                         \
                const size_t slot = (size_t)((e >> lgV) & (LANES - 1)) * VMAX + (size_t)(e & (V - 1));                     \
                for (int g = 0; g < n_cols; ++g) {                                                                         \
                    const T a = A ? A[c + (int64_t)g * m] : (T)1;                                                          \
                    T* a2 = acc2 + (size_t)g * LANES * VMAX + slot;                                                        \
                    T* a0 = acc0 + (size_t)g * LANES * VMAX + slot;                                                        \
                    *a2 = FMA(p, a, *a2);                                                                                  \
                    *a0 = *a0 + a;                                                                                         \
                }                                                                                                          \
            }                                                                                                              \
            for (int g = 0; g < n_cols; ++g) {                                                                             \
                S2[j + (int64_t)g * m] = reduce_##SUFFIX(acc2 + (size_t)g * LANES * VMAX, V);                              \
                S0[j + (int64_t)g * m] = reduce_##SUFFIX(acc0 + (size_t)g * LANES * VMAX, V);                              \
            }                                                                                                              \
        }                                                                                                                  \
        free(acc2);                                                                                                        \
        free(acc0);                                                                                                        \
        free(first);                                                                                                       \
        return rc;                                                                                                         \
    }

DEFINE_REPLAY(float, f32, fmaf)
DEFINE_REPLAY(double, f64, fma)
