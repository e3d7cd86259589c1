// Extremal eigenvalues of every LD block: one Lanczos recurrence per block, all blocks in lock step (include/viprs_hip.h,
// viprs_plan_extremal_eigenvalues).  An iteration is one LD product (ld_dot.h) and one launch of lanczos_step_kernel: one
// workgroup per LD block carries the block's vectors through
//     w = A v - fl(beta_k) v_prev,  alpha_k = v.w,  w -= fl(alpha_k) v,  beta_{k+1} = ||w||,  v_prev <- v,  v <- fl(w / beta_{k+1})
// and appends alpha_k, beta_{k+1} to the block's coefficient arrays; the host takes the Ritz values of the tridiagonal matrix
// and decides when a block stops (abi_spectrum.hip).  tests/lanczos_reference.py states the same recurrence on the host.
//
// NO REORTHOGONALISATION.  The Lanczos vectors lose their orthogonality as soon as a Ritz pair converges (Paige), and the
// tridiagonal matrix then grows ghost copies of eigenvalues it has already found.  The extremal Ritz values converge all the
// same, a ghost sits at an eigenvalue of A and so does no harm at either end of the spectrum, and beta_{k+1} |s_k| remains the
// residual norm of the Ritz vector to O(eps ||A||).  Two vectors per block instead of k.
//
// PRECISION and THE ORDER of the dot products are those of ridge.h, whose load / store / reduction helpers this file uses:
// vectors in the state precision T, every vector operation one rounded operation in T with its scalar coefficient rounded to
// T first, scalars and dot products in double; no floating-point atomics.  Every element is re-read by the thread that stored
// it, so the passes of a step need no barrier beyond the reductions'.
#pragma once
#include "ridge.h"

namespace viprs {

template <typename T> struct LanczosArgs {
    const RidgeBlock* blocks;  // SNP order
    double* beta;              // per block: beta_k on entry of step k, beta_{k+1} behind it
    int32_t* status;           // per block: kRidgeRunning / kRidgeConverged (beta_{k+1} == 0 here; the rest is the host's)
    int32_t* iters;            // per block: steps done
    int32_t* live;             // blocks still running
    const T* Y;                // A v of this iteration
    T* v;                      // Lanczos vector: read, then overwritten with the next one
    T* p;                      // v_prev on entry, w between the passes, v on exit
    double* alpha_out;         // [block * max_iter + k - 1]
    double* beta_out;
    int k, max_iter;
};

// u_i of the start vector: a function of the index inside the block alone
__host__ __device__ __forceinline__ double lanczos_start(int i) {
    unsigned long long h = (unsigned long long)(i + 1) * 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    h = h ^ (h >> 31);
    return (double)(h >> 40) * 0x1p-24 - 0.5 + 0x1p-25;
}

// v = fl(u / ||u||), v_prev = 0, beta_1 = 0
template <typename T>
__global__ __launch_bounds__(kRidgeThreads) void lanczos_init_kernel(LanczosArgs<T> A) {
    constexpr int V = ridge_vec<T>();
    __shared__ double red[kRidgeWaves];
    const RidgeBlock bd = A.blocks[blockIdx.x];
    const int size = bd.size;
    T* __restrict__ v = A.v + bd.start;
    T* __restrict__ p = A.p + bd.start;
    double part = 0.0;
    ridge_for_chunks<V>(size, [&](int e0, auto) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const double u = e0 + i < size ? lanczos_start(e0 + i) : 0.0;
            part = part + u * u;
        }
    });
    const double norm = sqrt(ridge_reduce(part, red));
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T o[V], z[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            o[i] = e0 + i < size ? (T)(lanczos_start(e0 + i) / norm) : (T)0;
            z[i] = (T)0;
        }
        ridge_store<T, V, FULL>(v, e0, size, o);
        ridge_store<T, V, FULL>(p, e0, size, z);
    });
    if (threadIdx.x == 0) {
        A.beta[blockIdx.x] = 0.0;
        A.status[blockIdx.x] = kRidgeRunning;
        A.iters[blockIdx.x] = 0;
    }
}

// One Lanczos step of every block that is still running.
template <typename T>
__global__ __launch_bounds__(kRidgeThreads) void lanczos_step_kernel(LanczosArgs<T> A) {
    constexpr int V = ridge_vec<T>();
    __shared__ double red[2][kRidgeWaves];
    if (A.status[blockIdx.x] != kRidgeRunning) return;      // final: nothing of this block changes any more
    const RidgeBlock bd = A.blocks[blockIdx.x];
    const int size = bd.size;
    const T bk = (T)A.beta[blockIdx.x];
    const T* __restrict__ Y = A.Y + bd.start;
    T* __restrict__ v = A.v + bd.start;
    T* __restrict__ p = A.p + bd.start;

    // pass A: w = A v - beta_k v_prev (into v_prev's place), alpha = v . w
    double part = 0.0;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T av[V], vv[V], pp[V], o[V];
        ridge_load<T, V, FULL>(Y, e0, size, av);
        ridge_load<T, V, FULL>(v, e0, size, vv);
        ridge_load<T, V, FULL>(p, e0, size, pp);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            o[i] = av[i] - bk * pp[i];
            part = part + (double)vv[i] * (double)o[i];
        }
        ridge_store<T, V, FULL>(p, e0, size, o);
    });
    const double alpha = ridge_reduce(part, red[0]);

    // pass B: w -= alpha v, beta_{k+1}^2 = w . w   (every thread re-reads what it stored itself)
    const T ak = (T)alpha;
    part = 0.0;
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T o[V], vv[V];
        ridge_load<T, V, FULL>(p, e0, size, o);
        ridge_load<T, V, FULL>(v, e0, size, vv);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            o[i] = o[i] - ak * vv[i];
            part = part + (double)o[i] * (double)o[i];
        }
        ridge_store<T, V, FULL>(p, e0, size, o);
    });
    const double nbeta = sqrt(ridge_reduce(part, red[1]));

    // (every read of the block's scalars above precedes the barrier inside the second reduction)
    if (threadIdx.x == 0) {
        const size_t at = (size_t)blockIdx.x * (size_t)A.max_iter + (size_t)(A.k - 1);
        A.alpha_out[at] = alpha;
        A.beta_out[at] = nbeta;
        A.beta[blockIdx.x] = nbeta;
        A.iters[blockIdx.x] = A.k;
        if (nbeta == 0.0) {                                 // an invariant subspace: T_k's eigenvalues are eigenvalues of A
            A.status[blockIdx.x] = kRidgeConverged;
            atomicSub(A.live, 1);
        }
    }
    if (nbeta == 0.0) return;                               // (no division by a vanished beta)

    // pass C: v_prev <- v, v <- w / beta_{k+1}
    ridge_for_chunks<V>(size, [&](int e0, auto full) {
        constexpr bool FULL = decltype(full)::value;
        T w[V], vv[V];
        ridge_load<T, V, FULL>(p, e0, size, w);
        ridge_load<T, V, FULL>(v, e0, size, vv);
        ridge_store<T, V, FULL>(p, e0, size, vv);
#pragma unroll
        for (int i = 0; i < V; ++i) w[i] = (T)((double)w[i] / nbeta);
        ridge_store<T, V, FULL>(v, e0, size, w);
    });
}

}  // namespace viprs
