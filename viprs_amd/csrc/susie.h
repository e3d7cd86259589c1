// SuSiE-RSS fine-mapping (Wang et al. 2020; Zou et al. 2022): z ~ N(R b, R), b = the sum of L single effects, one
// iterative Bayesian stepwise selection per LD block, all blocks in lock step (include/viprs_hip.h, viprs_plan_susie).
// A step -- effect l of iteration it -- is one launch of susie_step_kernel and one 1-column LD product (ld_dot.h): one
// workgroup per LD block stores the product of the step before (R bbar of effect l - 1) into its column of Rb, forms the
// residual z - sum_{l' != l} Rb[:, l'], the softmax of the log Bayes factors, the posterior means, the EM update of the
// effect's prior variance, and writes the product's next input column bbar = alpha mu.  tests/susie_replay.py states the
// same step on the host, operation by operation.
//
// PRECISION.  alpha, mu, Rb, bbar and the product are in the state precision T; z, log pi, the log Bayes factors w, the
// weights e and every scalar are doubles, formed from the stored T values.  exp is exp_glibc_f64_nonpos (device_math.h):
// the host libm's bits.  No contraction (-ffp-contract=off) and no fma in this file.
//
// THE ORDER of the two sums S and Q is the order of the ridge solve's dot products (ridge.h, whose chunk walkers and
// reduction this file uses): chunks of 16 bytes of T dealt to 256 threads in turn, one double accumulator per thread in
// ascending order, the xor butterfly over the 64 lanes, the wavefronts in order.  The maxima are order-free.  No
// floating-point atomics.  Every element is re-read by the thread that stored it, so the passes of a step need no barrier
// beyond the reductions'.
#pragma once
#include "device_math.h"
#include "ridge.h"

namespace viprs {

constexpr int kSusieMaxL = 32;

// scalars of one block, carried from launch to launch (V and post_var: (n_blocks, L) arrays of their own)
struct SusieRec {
    double delta;      // max |alpha - alpha_old| over the effects of the last completed iteration
    double delta_cur;  // ... over the effects of the iteration under way
    int32_t status;    // kRidgeRunning / kRidgeConverged / kRidgeMaxIter
    int32_t iters;     // completed iterations
};

template <typename T> struct SusieArgs {
    const RidgeBlock* blocks;  // SNP order
    SusieRec* rec;
    int32_t* live;             // blocks still running
    const T* Y;                // R bbar of the step before
    T* alpha;                  // (m, L) column-major
    T* mu;                     // (m, L)
    T* Rb;                     // (m, L): R (alpha_l mu_l)
    T* bbar;                   // (m,): the product's input
    double* w;                 // (m,): w between passes A and B, e between passes B and C
    const double* z;           // (m,)
    const double* log_pi;      // (m,)
    double* V;                 // (n_blocks, L) prior variances
    double* post_var;          // (n_blocks, L)
    const double* V0;          // init only: the start of V
    int64_t m;
    double tol;
    int L, l, it, max_iter;
    int store_prev;            // every step but the call's first: Rb[:, (l - 1) mod L] = Y
    int estimate;              // EM update of V
};

// the workgroup's maximum of `t`; every thread returns it.  `slots` as for ridge_reduce.
__device__ __forceinline__ double susie_reduce_max(double t, double* slots) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        const double o = __shfl_xor(t, w, 64);
        t = o > t ? o : t;
    }
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = t;
    __syncthreads();
    double s = slots[0];
#pragma unroll
    for (int k = 1; k < kRidgeWaves; ++k) s = slots[k] > s ? slots[k] : s;
    return s;
}

// alpha = mu = Rb = 0, V = V0, every block running
template <typename T>
__global__ __launch_bounds__(kRidgeThreads) void susie_init_kernel(SusieArgs<T> A) {
    constexpr int V = ridge_vec<T>();
    const RidgeBlock bd = A.blocks[blockIdx.x];
    const int size = bd.size;
    T zero[V];
#pragma unroll
    for (int i = 0; i < V; ++i) zero[i] = (T)0;
    for (int l = 0; l < A.L; ++l) {
        const int64_t col = (int64_t)l * A.m + bd.start;
        T* __restrict__ a = A.alpha + col;
        T* __restrict__ mu = A.mu + col;
        T* __restrict__ rb = A.Rb + col;
        ridge_for_chunks<V>(size, [&](int e0, auto full) {
            constexpr bool FULL = decltype(full)::value;
            ridge_store<T, V, FULL>(a, e0, size, zero);
            ridge_store<T, V, FULL>(mu, e0, size, zero);
            ridge_store<T, V, FULL>(rb, e0, size, zero);
        });
    }
    for (int l = (int)threadIdx.x; l < A.L; l += kRidgeThreads) {
        const size_t at = (size_t)blockIdx.x * (size_t)A.L + (size_t)l;
        A.V[at] = A.V0[at];
        A.post_var[at] = 0.0;
    }
    if (threadIdx.x == 0) {
        SusieRec r;
        r.delta = 0.0;
        r.delta_cur = 0.0;
        r.status = kRidgeRunning;
        r.iters = 0;
        A.rec[blockIdx.x] = r;
        atomicAdd(A.live, 1);
    }
}

// Effect A.l of iteration A.it of every block that is still running.
template <typename T>
__global__ __launch_bounds__(kRidgeThreads) void susie_step_kernel(SusieArgs<T> A) {
    constexpr int V = ridge_vec<T>();
    __shared__ double red[4][kRidgeWaves];
    SusieRec* rec = A.rec + blockIdx.x;
    if (rec->status != kRidgeRunning) return;       // final: nothing of this block changes any more
    const RidgeBlock bd = A.blocks[blockIdx.x];
    const int size = bd.size;
    const int L = A.L, l = A.l;
    const int lprev = l == 0 ? L - 1 : l - 1;
    const bool store_prev = A.store_prev != 0;
    const size_t at = (size_t)blockIdx.x * (size_t)L + (size_t)l;
    const double Vl = A.V[at];
    const double s = Vl / (1.0 + Vl);
    const T* __restrict__ Y = A.Y + bd.start;
    T* __restrict__ Rb = A.Rb + bd.start;           // column l' at Rb + l' m
    T* __restrict__ alpha = A.alpha + (int64_t)l * A.m + bd.start;
    T* __restrict__ mu = A.mu + (int64_t)l * A.m + bd.start;
    T* __restrict__ bbar = A.bbar + bd.start;
    double* __restrict__ w = A.w + bd.start;
    const double* __restrict__ z = A.z + bd.start;
    const double* __restrict__ lp = A.log_pi + bd.start;

    // pass A: Rb[:, l - 1] = Y;  r = z - sum_{l' != l} Rb[:, l'];  w = 0.5 r^2 s + log pi;  mu = s r;  wmax = max w
    double wmax = -__builtin_inf();
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        double acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = 0.0;
        T y[V];
        if (store_prev) {
            ridge_load<T, V, FULL>(Y, e0, size, y);
            ridge_store<T, V, FULL>(Rb + (int64_t)lprev * A.m, e0, size, y);
        }
        for (int k = 0; k < L; ++k) {               // ascending l'
            if (k == l) continue;
            T c[V];
            if (store_prev && k == lprev) {         // (what was stored above)
#pragma unroll
                for (int i = 0; i < V; ++i) c[i] = y[i];
            } else {
                ridge_load<T, V, FULL>(Rb + (int64_t)k * A.m, e0, size, c);
            }
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] = acc[i] + (double)c[i];
        }
        T m_[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            m_[i] = (T)0;
            if (FULL || e0 + i < size) {
                const double r = z[e0 + i] - acc[i];
                const double wi = (0.5 * (r * r)) * s + lp[e0 + i];
                m_[i] = (T)(s * r);
                w[e0 + i] = wi;
                wmax = wi > wmax ? wi : wmax;
            }
        }
        ridge_store<T, V, FULL>(mu, e0, size, m_);
    });
    wmax = susie_reduce_max(wmax, red[0]);

    // pass B: e = exp(w - wmax), S = sum e, Q = sum e (s + mu^2)
    double ps = 0.0, pq = 0.0;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T m_[V];
        ridge_load<T, V, FULL>(mu, e0, size, m_);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            if (FULL || e0 + i < size) {
                const double e = exp_glibc_f64_nonpos(w[e0 + i] - wmax);
                const double md = (double)m_[i];
                ps = ps + e;
                pq = pq + e * (s + md * md);
                w[e0 + i] = e;
            }
        }
    });
    const double S = ridge_reduce(ps, red[1]);
    const double Q = ridge_reduce(pq, red[2]);

    // pass C: alpha = e / S, bbar = alpha mu, delta = max |alpha - alpha_old|
    double dmax = 0.0;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T m_[V], a[V], b[V];
        ridge_load<T, V, FULL>(mu, e0, size, m_);
        ridge_load<T, V, FULL>(alpha, e0, size, a);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            b[i] = (T)0;
            if (FULL || e0 + i < size) {
                const T an = (T)(w[e0 + i] / S);
                const double d = fabs((double)an - (double)a[i]);
                dmax = d > dmax ? d : dmax;
                b[i] = (T)((double)an * (double)m_[i]);
                a[i] = an;
            }
        }
        ridge_store<T, V, FULL>(alpha, e0, size, a);
        ridge_store<T, V, FULL>(bbar, e0, size, b);
    });
    dmax = susie_reduce_max(dmax, red[3]);

    // (every thread read V[l] and the status before the barriers of the reductions)
    if (threadIdx.x == 0) {
        A.post_var[at] = s;
        if (A.estimate) A.V[at] = Q / S;
        const double dc = l == 0 ? dmax : (dmax > rec->delta_cur ? dmax : rec->delta_cur);
        rec->delta_cur = dc;
        if (l == L - 1) {
            int32_t status = kRidgeRunning;
            if (dc < A.tol) status = kRidgeConverged;
            else if (A.it >= A.max_iter) status = kRidgeMaxIter;
            rec->delta = dc;
            rec->iters = A.it;
            rec->status = status;
            if (status != kRidgeRunning) atomicSub(A.live, 1);
        }
    }
}

}  // namespace viprs
