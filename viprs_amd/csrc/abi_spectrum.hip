// C ABI, extremal eigenvalues (include/viprs_hip.h): lambda_min and lambda_max of every LD block by one Lanczos recurrence
// per block, all blocks in lock step -- what `lambda_min='infer'` (viprs/model/VIPRS.py:174-191) needs from the LD matrix.
// Kernels: lanczos.h; the product of every iteration: abi_dot.hip; the stopping rule: here, on the host.
#include <atomic>
#include <cmath>
#include <thread>

#include "internal.h"
#include "lanczos.h"

using namespace viprs;

namespace {

// Extreme eigenpairs of the symmetric tridiagonal matrix with diagonal a[0..n-1] and off-diagonal b[0..n-2] by the implicit
// QL iteration (EISPACK tql2), carrying only the LAST ROW z of the eigenvector matrix: a rotation of the columns (i, i + 1)
// treats every row alike, so the last row can be carried alone -- O(n^2) operations, O(n) memory.  out: theta_min,
// theta_max, |z| of theta_min, |z| of theta_max.
void tridiagonal_extremes(int n, const double* a, const double* b, double* out) {
    std::vector<double> d(a, a + n), e((size_t)n, 0.0), z((size_t)n, 0.0);
    for (int i = 0; i + 1 < n; ++i) e[(size_t)i] = b[i];
    z[(size_t)n - 1] = 1.0;
    const double eps = 2.220446049250313e-16;
    double f = 0.0, tst1 = 0.0;
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n - 1 && !(std::fabs(e[m]) <= eps * tst1)) ++m;
        if (m > l) {
            int iter = 0;
            do {
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c;
                const double el1 = e[l + 1];
                double s = 0.0, s2 = 0.0;
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = std::hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    h = z[i + 1];
                    z[i + 1] = s * z[i] + c * h;
                    z[i] = c * z[i] - s * h;
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1 && ++iter < 100);
        }
        d[l] += f;
        e[l] = 0.0;
    }
    int lo = 0, hi = 0;
    for (int i = 1; i < n; ++i) {
        if (d[i] < d[lo]) lo = i;
        if (d[i] > d[hi]) hi = i;
    }
    out[0] = d[lo];
    out[1] = d[hi];
    out[2] = std::fabs(z[lo]);
    out[3] = std::fabs(z[hi]);
}

int build_spectrum_workspace(viprs_plan* P, size_t elem, int max_iter) {
    SpectrumWork& W = P->spectrum;
    const size_t nb = P->blocks.size();
    int rc = ensure_solver_blocks(P);
    if (rc != VIPRS_OK) return rc;
    if (!W.built) {
        HIP_TRY(W.d_beta.alloc(nb));
        HIP_TRY(W.d_status.alloc(nb));
        HIP_TRY(W.d_iters.alloc(nb));
        HIP_TRY(W.d_live.alloc(1));
        W.built = true;
    }
    const size_t bytes = (size_t)P->m * elem;
    if (W.vec_bytes < bytes) {
        W.vec_bytes = 0;
        for (auto& v : W.d_vec) HIP_TRY(v.alloc(bytes));
        W.vec_bytes = bytes;
    }
    const size_t coef = nb * (size_t)max_iter;
    if (W.coef_cap < coef) {
        W.coef_cap = 0;
        HIP_TRY(W.d_alpha.alloc(coef));
        HIP_TRY(W.d_betas.alloc(coef));
        W.coef_cap = coef;
    }
    return VIPRS_OK;
}

struct SpectrumOut {
    std::vector<double> lo, hi, r_lo, r_hi;
    std::vector<int32_t> iters, status;
};

// body(i) for i in [0, n) on up to 8 host threads when the work is worth them; every i is independent
template <typename F> void parallel_blocks(const std::vector<size_t>& items, double work, F&& body) {
    const unsigned want = work < 4e6 ? 1u : std::min<unsigned>({8u, std::max(1u, std::thread::hardware_concurrency()),
                                                               (unsigned)items.size()});
    if (want <= 1) {
        for (size_t i : items) body(i);
        return;
    }
    std::atomic<size_t> next{0};
    auto run = [&] {
        for (size_t j = next.fetch_add(1); j < items.size(); j = next.fetch_add(1)) body(items[j]);
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < want; ++t) pool.emplace_back(run);
    run();
    for (auto& t : pool) t.join();
}

template <typename T>
int spectrum_typed(viprs_plan* P, int float_dtype, double dq_scale, double rtol, int max_iter, SpectrumOut& O) {
    SpectrumWork& W = P->spectrum;
    const size_t nb = P->blocks.size();
    T* v = reinterpret_cast<T*>(W.d_vec[0].p);
    T* p = reinterpret_cast<T*>(W.d_vec[1].p);
    T* Y = reinterpret_cast<T*>(W.d_vec[2].p);

    LanczosArgs<T> A;
    A.blocks = P->d_solver_blocks.p;
    A.beta = W.d_beta.p;
    A.status = W.d_status.p;
    A.iters = W.d_iters.p;
    A.live = W.d_live.p;
    A.Y = Y;
    A.v = v;
    A.p = p;
    A.alpha_out = W.d_alpha.p;
    A.beta_out = W.d_betas.p;
    A.k = 0;
    A.max_iter = max_iter;

    int32_t live = (int32_t)nb;
    HIP_TRY(hipMemcpyAsync(W.d_live.p, &live, sizeof(live), hipMemcpyHostToDevice, P->stream));
    HIP_TRY(hipStreamSynchronize(P->stream));           // (`live` above is a local)
    int rc = W.time.start(P->stream);
    if (rc != VIPRS_OK) return rc;
    lanczos_init_kernel<T><<<(unsigned)nb, kRidgeThreads, 0, P->stream>>>(A);
    HIP_TRY(hipGetLastError());

    O.lo.assign(nb, 0.0); O.hi.assign(nb, 0.0); O.r_lo.assign(nb, 0.0); O.r_hi.assign(nb, 0.0);
    O.iters.assign(nb, 0); O.status.assign(nb, kRidgeRunning);
    std::vector<std::vector<double>> al(nb), be(nb);     // the coefficients of the blocks that are still running
    std::vector<int32_t> dev_status(nb), dev_iters(nb);
    std::vector<double> stage_a, stage_b;
    std::vector<size_t> running;
    W.iterations = 0;
    W.host_ms = 0.0;
    int k_prev = 0, next_check = 1;
    size_t n_running = nb;
    for (int k = 1; k <= max_iter && n_running > 0; ++k) {
        rc = enqueue_dot(P, float_dtype, 1, v, Y, dq_scale, 1);
        if (rc != VIPRS_OK) return rc;
        A.k = k;
        lanczos_step_kernel<T><<<(unsigned)nb, kRidgeThreads, 0, P->stream>>>(A);
        HIP_TRY(hipGetLastError());
        W.iterations = k;
        if (k != next_check && k != max_iter) continue;

        // the stopping rule: the coefficients since the last check, then the extreme Ritz pairs of every running block
        HIP_TRY(hipStreamSynchronize(P->stream));
        const double t0 = host_clock_ms();
        const size_t cols = (size_t)(k - k_prev);
        stage_a.resize(nb * cols);
        stage_b.resize(nb * cols);
        HIP_TRY(hipMemcpy(dev_status.data(), W.d_status.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(dev_iters.data(), W.d_iters.p, nb * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy2D(stage_a.data(), cols * sizeof(double), W.d_alpha.p + k_prev, (size_t)max_iter * sizeof(double),
                            cols * sizeof(double), nb, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy2D(stage_b.data(), cols * sizeof(double), W.d_betas.p + k_prev, (size_t)max_iter * sizeof(double),
                            cols * sizeof(double), nb, hipMemcpyDeviceToHost));
        running.clear();
        double work = 0.0;
        for (size_t b = 0; b < nb; ++b) {
            if (O.status[b] != kRidgeRunning) continue;
            const int n = std::min(std::max(dev_iters[b], k_prev), k);      // (< k: beta vanished on the way)
            al[b].insert(al[b].end(), stage_a.begin() + b * cols, stage_a.begin() + b * cols + (size_t)(n - k_prev));
            be[b].insert(be[b].end(), stage_b.begin() + b * cols, stage_b.begin() + b * cols + (size_t)(n - k_prev));
            running.push_back(b);
            work += (double)n * (double)n;
        }
        parallel_blocks(running, work, [&](size_t b) {
            const int n = (int)al[b].size();
            double r[4];
            tridiagonal_extremes(n, al[b].data(), be[b].data(), r);
            const double res = be[b][(size_t)n - 1];
            const double scale = std::max(std::fabs(r[0]), std::fabs(r[1]));
            O.lo[b] = r[0];
            O.hi[b] = r[1];
            O.r_lo[b] = res * r[2];
            O.r_hi[b] = res * r[3];
            O.iters[b] = n;
            if (dev_status[b] != kRidgeRunning || res == 0.0 || (O.r_lo[b] <= rtol * scale && O.r_hi[b] <= rtol * scale))
                O.status[b] = kRidgeConverged;
            else if (k >= max_iter)
                O.status[b] = kRidgeMaxIter;
        });
        n_running = 0;
        for (size_t b : running) {
            if (O.status[b] == kRidgeRunning) { ++n_running; continue; }
            std::vector<double>().swap(al[b]);
            std::vector<double>().swap(be[b]);
        }
        // the blocks that stopped are frozen on the device too
        live = (int32_t)n_running;
        HIP_TRY(hipMemcpy(W.d_status.p, O.status.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(W.d_live.p, &live, sizeof(live), hipMemcpyHostToDevice));
        W.host_ms += host_clock_ms() - t0;
        k_prev = k;
        next_check *= 2;
    }
    rc = W.time.stop(P->stream);
    if (rc != VIPRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(P->stream));
    return check_device_error(P);
}

}  // namespace

extern "C" {

int viprs_plan_extremal_eigenvalues(viprs_plan* P, int float_dtype, double dq_scale, double rtol, int max_iter,
                                    double* lam_min, double* lam_max, double* resid_min, double* resid_max,
                                    int32_t* block_iters, int32_t* block_status) {
    if (!P) return fail(VIPRS_EINVAL, "null plan");
    const size_t elem = float_size(float_dtype);
    if (elem == 0) return fail(VIPRS_EINVAL, "bad float dtype code");
    if (!(rtol > 0.0)) return fail(VIPRS_EINVAL, "rtol must be positive");
    if (max_iter < 1) return fail(VIPRS_EINVAL, "max_iter must be at least 1");
    if (P->m == 0) return VIPRS_OK;
    HIP_TRY(hipSetDevice(P->device));
    int rc = build_spectrum_workspace(P, elem, max_iter);
    if (rc != VIPRS_OK) return rc;
    SpectrumOut O;
    if (float_dtype == VIPRS_F32) rc = spectrum_typed<float>(P, float_dtype, dq_scale, rtol, max_iter, O);
    else rc = spectrum_typed<double>(P, float_dtype, dq_scale, rtol, max_iter, O);
    if (rc != VIPRS_OK) return rc;
    for (size_t k = 0; k < P->blocks.size(); ++k) {
        if (lam_min) lam_min[k] = O.lo[k];
        if (lam_max) lam_max[k] = O.hi[k];
        if (resid_min) resid_min[k] = O.r_lo[k];
        if (resid_max) resid_max[k] = O.r_hi[k];
        if (block_iters) block_iters[k] = O.iters[k];
        if (block_status) block_status[k] = O.status[k];
    }
    return VIPRS_OK;
}

int viprs_plan_last_spectrum_ms(viprs_plan* P, double* total_ms, int* iterations, double* host_ms) {
    if (!P || !total_ms) return fail(VIPRS_EINVAL, "null argument");
    const int rc = P->spectrum.time.elapsed(P->device, total_ms, "no timed spectrum yet");
    if (rc != VIPRS_OK) return rc;
    if (iterations) *iterations = P->spectrum.iterations;
    if (host_ms) *host_ms = P->spectrum.host_ms;
    return VIPRS_OK;
}

int viprs_tridiagonal_extremes(int k, const double* alpha, const double* beta, double* out) {
    if (k < 1 || !alpha || !out || (k > 1 && !beta)) return fail(VIPRS_EINVAL, "bad tridiagonal matrix");
    tridiagonal_extremes(k, alpha, beta, out);
    return VIPRS_OK;
}

}  // extern "C"
