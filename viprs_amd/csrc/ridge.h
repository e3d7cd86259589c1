// Ridge solve (R + diag(shift)) x = b, one independent MINRES (Paige & Saunders 1975) per LD block, all blocks in lock step
// (include/viprs_hip.h, viprs_plan_solve_ridge).  An iteration is one LD product (ld_dot.h) and one launch of
// ridge_step_kernel: one workgroup per LD block carries the block's vectors through the Lanczos step, the Givens rotation
// and the update of the solution.  tests/ridge_reference.py states the same recurrences on the host.
//
// PRECISION.  Vectors are in the state precision T and every vector operation is one rounded operation in T with its scalar
// coefficient rounded to T first; the per-block scalars and every dot product are in double.
//
// THE ORDER of a dot product over a block of `size` SNPs, V = 16 / sizeof(T): element e belongs to chunk e / V, chunk c to
// thread c % kRidgeThreads; a thread adds the products of its elements to ONE double accumulator in ascending e, the 64
// lanes of a wavefront are summed by an xor butterfly (6 levels), the wavefronts' sums in wavefront order.  A function of
// the block's size alone: not of the block's place in the plan, of the other blocks or of timing.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace viprs {

constexpr int kRidgeThreads = 256;
constexpr int kRidgeWaves = kRidgeThreads / 64;

enum { kRidgeRunning = -1, kRidgeConverged = 0, kRidgeMaxIter = 1, kRidgeZeroRhs = 2 };

struct RidgeBlock {
    int64_t start;     // first SNP
    int32_t size;
    int32_t pad_;
};

// scalars of one block's MINRES, carried from launch to launch
struct RidgeRec {
    double bnorm;      // ||b||: what the stopping rule and relres are relative to (= beta1 without a start vector)
    double beta, oldb, dbar, epsln, phibar, cs, sn;
    int32_t status;    // kRidge*
    int32_t iters;
};

template <typename T> struct RidgeArgs {
    const RidgeBlock* blocks;  // SNP order
    RidgeRec* rec;
    int32_t* live;             // blocks still running
    const T* Y;                // R v of this iteration (init: R x0)
    const T* shift;
    T* v;                      // Lanczos vector: read, then overwritten with the next one
    const T* r1;
    const T* r2;               // (init: b on entry)
    T* y;                      // the new r2
    const T* w1;
    const T* w2;
    T* w;
    T* x;
    double rtol;
    int itn, max_iter;
    int has_x0;                // init only
};

template <typename T> constexpr int ridge_vec() { return 16 / (int)sizeof(T); }

// V consecutive elements from p[e0 ..]: one 16-byte access for a whole chunk (FULL), element by element (zeros beyond the
// block's end) for the block's last, partial chunk
template <typename T, int V, bool FULL>
__device__ __forceinline__ void ridge_load(const T* __restrict__ p, int e0, int size, T (&o)[V]) {
    if constexpr (FULL) {
        __builtin_memcpy(o, p + e0, sizeof(T) * V);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) o[i] = e0 + i < size ? p[e0 + i] : (T)0;
    }
}
template <typename T, int V, bool FULL>
__device__ __forceinline__ void ridge_store(T* __restrict__ p, int e0, int size, const T (&o)[V]) {
    if constexpr (FULL) {
        __builtin_memcpy(p + e0, o, sizeof(T) * V);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (e0 + i < size) p[e0 + i] = o[i];
    }
}

// the workgroup's sum of `t` in THE ORDER above; every thread returns it.  `slots`: kRidgeWaves doubles of LDS nobody else
// touches until the next barrier behind this call.
__device__ __forceinline__ double ridge_reduce(double t, double* slots) {
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) t = t + __shfl_xor(t, w, 64);
    if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = t;
    __syncthreads();
    double s = slots[0];
#pragma unroll
    for (int k = 1; k < kRidgeWaves; ++k) s = s + slots[k];
    return s;
}

// the chunks of a block that belong to this thread, in ascending order: whole chunks, then the block's partial last chunk
template <int V, typename F>
__device__ __forceinline__ void ridge_for_chunks(int size, F&& body) {
    for (int e0 = (int)threadIdx.x * V; e0 + V <= size; e0 += kRidgeThreads * V) body(e0, std::true_type{});
    const int et = size - size % V;
    if (et < size && (et / V) % kRidgeThreads == (int)threadIdx.x) body(et, std::false_type{});
}

// r2 = y = b - (R + diag(shift)) x0 (b itself without x0), r1 = y, beta1 = ||y||, the first v = y / beta1.
// A block with b = 0 is final at once (x = 0), so is one whose start vector already meets the tolerance.
template <typename T>
__global__ __launch_bounds__(kRidgeThreads) void ridge_init_kernel(RidgeArgs<T> A, T* r1_out) {
    constexpr int V = ridge_vec<T>();
    __shared__ double red[2][kRidgeWaves];
    const RidgeBlock bd = A.blocks[blockIdx.x];
    const int size = bd.size;
    const T* __restrict__ Y = A.Y + bd.start;
    const T* __restrict__ sh = A.shift + bd.start;
    T* __restrict__ x = A.x + bd.start;
    T* __restrict__ r1 = r1_out + bd.start;
    T* __restrict__ r2 = A.y + bd.start;
    T* __restrict__ v = A.v + bd.start;
    const bool has_x0 = A.has_x0 != 0;
    double bb = 0.0, yy = 0.0;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T b[V], y[V];
        ridge_load<T, V, FULL>(r2, e0, size, b);
        if (has_x0) {
            T ax[V], s[V], x0[V];
            ridge_load<T, V, FULL>(Y, e0, size, ax);
            ridge_load<T, V, FULL>(sh, e0, size, s);
            ridge_load<T, V, FULL>(x, e0, size, x0);
#pragma unroll
            for (int i = 0; i < V; ++i) y[i] = b[i] - (ax[i] + s[i] * x0[i]);
            ridge_store<T, V, FULL>(r2, e0, size, y);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) y[i] = b[i];
        }
        ridge_store<T, V, FULL>(r1, e0, size, y);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            bb = bb + (double)b[i] * (double)b[i];
            yy = yy + (double)y[i] * (double)y[i];
        }
    });
    bb = ridge_reduce(bb, red[0]);
    yy = ridge_reduce(yy, red[1]);
    const double bnorm = sqrt(bb), beta1 = sqrt(yy);
    int32_t status = kRidgeRunning;
    if (bnorm == 0.0) status = kRidgeZeroRhs;
    else if (beta1 <= A.rtol * bnorm) status = kRidgeConverged;
    if (threadIdx.x == 0) {
        RidgeRec r;
        r.bnorm = bnorm;
        r.beta = beta1;
        r.oldb = 0.0;
        r.dbar = 0.0;
        r.epsln = 0.0;
        r.phibar = status == kRidgeZeroRhs ? 0.0 : beta1;
        r.cs = -1.0;
        r.sn = 0.0;
        r.status = status;
        r.iters = 0;
        A.rec[blockIdx.x] = r;
        if (status == kRidgeRunning) atomicAdd(A.live, 1);
    }
    if (status == kRidgeConverged) return;
    const bool zero = status == kRidgeZeroRhs;
    const T b1 = (T)beta1;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T o[V];
        if (zero) {
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] = (T)0;
            ridge_store<T, V, FULL>(x, e0, size, o);
        } else {
            ridge_load<T, V, FULL>(r2, e0, size, o);          // (this thread's own stores)
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] = o[i] / b1;
            ridge_store<T, V, FULL>(v, e0, size, o);
        }
    });
}

// One MINRES iteration of every block that is still running.
template <typename T>
__global__ __launch_bounds__(kRidgeThreads) void ridge_step_kernel(RidgeArgs<T> A) {
    constexpr int V = ridge_vec<T>();
    __shared__ double red[2][kRidgeWaves];
    __shared__ double sc[5];
    __shared__ int32_t s_final;
    RidgeRec* rec = A.rec + blockIdx.x;
    if (rec->status != kRidgeRunning) return;       // final: nothing of this block changes any more
    const RidgeBlock bd = A.blocks[blockIdx.x];
    const int size = bd.size;
    const double beta = rec->beta, oldb = rec->oldb;
    const T* __restrict__ Y = A.Y + bd.start;
    const T* __restrict__ sh = A.shift + bd.start;
    T* __restrict__ v = A.v + bd.start;
    const T* __restrict__ r1 = A.r1 + bd.start;
    const T* __restrict__ r2 = A.r2 + bd.start;
    T* __restrict__ y = A.y + bd.start;
    const T* __restrict__ w1 = A.w1 + bd.start;
    const T* __restrict__ w2 = A.w2 + bd.start;
    T* __restrict__ w = A.w + bd.start;
    T* __restrict__ x = A.x + bd.start;

    // pass A: y = (R + diag(shift)) v - (beta / oldb) r1, alfa = v . y
    const bool second = A.itn >= 2;
    const T c1 = second ? (T)(beta / oldb) : (T)0;
    double part = 0.0;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T av[V], s[V], vv[V], o[V];
        ridge_load<T, V, FULL>(Y, e0, size, av);
        ridge_load<T, V, FULL>(sh, e0, size, s);
        ridge_load<T, V, FULL>(v, e0, size, vv);
#pragma unroll
        for (int i = 0; i < V; ++i) o[i] = av[i] + s[i] * vv[i];
        if (second) {
            T p[V];
            ridge_load<T, V, FULL>(r1, e0, size, p);
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] = o[i] - c1 * p[i];
        }
#pragma unroll
        for (int i = 0; i < V; ++i) part = part + (double)vv[i] * (double)o[i];
        ridge_store<T, V, FULL>(y, e0, size, o);
    });
    const double alfa = ridge_reduce(part, red[0]);

    // pass B: y -= (alfa / beta) r2, beta^2 = y . y   (every thread re-reads what it stored itself)
    const T c2 = (T)(alfa / beta);
    part = 0.0;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T o[V], p[V];
        ridge_load<T, V, FULL>(y, e0, size, o);
        ridge_load<T, V, FULL>(r2, e0, size, p);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            o[i] = o[i] - c2 * p[i];
            part = part + (double)o[i] * (double)o[i];
        }
        ridge_store<T, V, FULL>(y, e0, size, o);
    });
    const double bb = ridge_reduce(part, red[1]);

    // the rotation, by one thread (every read of the record above precedes the barrier inside the second reduction)
    if (threadIdx.x == 0) {
        const double nbeta = sqrt(bb);
        const double oldeps = rec->epsln, dbar = rec->dbar, cs = rec->cs, sn = rec->sn, phibar = rec->phibar;
        const double delta = cs * dbar + sn * alfa;
        const double gbar = sn * dbar - cs * alfa;
        double gamma = sqrt(gbar * gbar + nbeta * nbeta);
        if (!(gamma > 2.220446049250313e-16)) gamma = 2.220446049250313e-16;
        const double ncs = gbar / gamma, nsn = nbeta / gamma;
        const double phi = ncs * phibar, nphibar = nsn * phibar;
        int32_t status = kRidgeRunning;
        if (nphibar <= A.rtol * rec->bnorm || nbeta == 0.0) status = kRidgeConverged;
        else if (A.itn >= A.max_iter) status = kRidgeMaxIter;
        rec->oldb = beta;
        rec->beta = nbeta;
        rec->epsln = sn * nbeta;                      // (the rotation of the iteration before, not this one's)
        rec->dbar = -cs * nbeta;
        rec->cs = ncs;
        rec->sn = nsn;
        rec->phibar = nphibar;
        rec->iters = A.itn;
        rec->status = status;
        if (status != kRidgeRunning) atomicSub(A.live, 1);
        sc[0] = oldeps; sc[1] = delta; sc[2] = gamma; sc[3] = phi; sc[4] = nbeta;
        s_final = status != kRidgeRunning;
    }
    __syncthreads();

    // pass C: w = (v - oldeps w1 - delta w2) / gamma, x += phi w, the next v = y / beta
    const T oe = (T)sc[0], de = (T)sc[1], ga = (T)sc[2], ph = (T)sc[3], nb = (T)sc[4];
    const bool last = s_final != 0;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T vv[V], a[V], b[V], xx[V], o[V];
        ridge_load<T, V, FULL>(v, e0, size, vv);
        ridge_load<T, V, FULL>(w1, e0, size, a);
        ridge_load<T, V, FULL>(w2, e0, size, b);
        ridge_load<T, V, FULL>(x, e0, size, xx);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            o[i] = ((vv[i] - oe * a[i]) - de * b[i]) / ga;
            xx[i] = xx[i] + ph * o[i];
        }
        ridge_store<T, V, FULL>(w, e0, size, o);
        ridge_store<T, V, FULL>(x, e0, size, xx);
        if (!last) {                                  // (a final block is never multiplied again: no division by a vanished beta)
            ridge_load<T, V, FULL>(y, e0, size, o);
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] = o[i] / nb;
            ridge_store<T, V, FULL>(v, e0, size, o);
        }
    });
}

}  // namespace viprs
