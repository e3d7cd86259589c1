/* TEST INFRASTRUCTURE ONLY: the SBayesR sweep of include/viprs_hip.h (viprs_state_bayesr_sweep) replayed on the host with the
 * draws handed in, written from the header's text.  Built at test time by tests/bayesr_replay.py with -O2 -ffp-contract=off:
 * every operation below is rounded on its own; the fused multiply-adds the header names go through libm's fmaf, expf is
 * libm's.  The walk over the rows, the axpy, the symmetric form's diagonal term and the upper form's second pass are those of
 * e_step.hpp:387-442 (as tests/gibbs_replay.c); only the update of one SNP differs. */
#include <math.h>
#include <stdint.h>

#define BAYESR_MAX_K 4

#define BAYESR_SWEEP(SUF, U)                                                                                            \
    int bayesr_replay_sweep_##SUF(int64_t m, int K, const int32_t* lb, const int64_t* ip, const U* ld, int low_memory,   \
                                  const float* std_beta, const float* mu_mult, const float* shvt, const float* u_logs,   \
                                  const float* log_null_pi, const float* unif, const float* z, float* eta, float* q,     \
                                  float* eta_diff, float* var_mu, float* var_gamma, int32_t* kstar, float dq) {          \
        if (m < 0 || K < 1 || K > BAYESR_MAX_K || !lb || !ip || !std_beta || !mu_mult || !shvt || !u_logs ||             \
            !log_null_pi || !unif || !z || !eta || !q || !eta_diff || !var_mu || !var_gamma || !kstar)                   \
            return -1;                                                                                                  \
        for (int64_t j = 0; j < m; ++j) {                                                                               \
            float mu[BAYESR_MAX_K], u[BAYESR_MAX_K], gam[BAYESR_MAX_K];                                                   \
            const float r = std_beta[j] - q[j];                                                                         \
            float mx = log_null_pi[j];                                                                                  \
            for (int k = 0; k < K; ++k) {                                                                               \
                mu[k] = mu_mult[j * K + k] * r;                                                                         \
                const float t = shvt[j * K + k] * mu[k];                                                                \
                u[k] = fmaf(t, t, u_logs[j * K + k]);                                                                   \
                mx = fmaxf(mx, u[k]);                                                                                   \
            }                                                                                                           \
            float ssum = 0.0f;                                                                                          \
            for (int k = 0; k < K; ++k) {                                                                               \
                u[k] = expf(u[k] - mx);                                                                                 \
                ssum += u[k];                                                                                           \
            }                                                                                                           \
            ssum += expf(log_null_pi[j] - mx);                                                                          \
            float c = 0.0f, b = 0.0f;                                                                                   \
            int ks = 0;                                                                                                 \
            for (int k = 0; k < K; ++k) {                                                                               \
                gam[k] = u[k] / ssum;                                                                                   \
                c = k == 0 ? gam[k] : c + gam[k];                                                                       \
                if (ks == 0 && unif[j] < c) {                                                                           \
                    const float sd = 0x1.6a09e6p-1f / shvt[j * K + k];                                                  \
                    const float n = z[j] * sd;                                                                          \
                    b = mu[k] + n;                                                                                      \
                    ks = k + 1;                                                                                         \
                }                                                                                                       \
            }                                                                                                           \
            const float d = b - eta[j];                                                                                 \
            for (int k = 0; k < K; ++k) {                                                                               \
                var_mu[j * K + k] = mu[k];                                                                              \
                var_gamma[j * K + k] = gam[k];                                                                          \
            }                                                                                                           \
            eta_diff[j] = d;                                                                                            \
            kstar[j] = ks;                                                                                              \
            const float alpha = dq * d;                                                                                 \
            float* x = q + lb[j];                                                                                       \
            const U* y = ld + ip[j];                                                                                    \
            const int64_t len = ip[j + 1] - ip[j];                                                                      \
            for (int64_t i = 0; i < len; ++i) x[i] = fmaf((float)y[i], alpha, x[i]);                                    \
            if (!low_memory) q[j] -= d;                                                                                 \
            eta[j] = b;                                                                                                 \
        }                                                                                                               \
        if (low_memory) {                                                                                               \
            for (int64_t j = 0; j < m; ++j) {                                                                           \
                const float* x = eta_diff + lb[j];                                                                      \
                const U* y = ld + ip[j];                                                                                \
                const int64_t len = ip[j + 1] - ip[j];                                                                  \
                float s = 0.0f;                                                                                         \
                for (int64_t i = 0; i < len; ++i) s = fmaf((float)y[i], x[i], s);                                       \
                q[j] += dq * s;                                                                                         \
            }                                                                                                           \
        }                                                                                                               \
        return 0;                                                                                                       \
    }

BAYESR_SWEEP(f32, float)
BAYESR_SWEEP(i8, int8_t)
BAYESR_SWEEP(i16, int16_t)
