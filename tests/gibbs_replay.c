/* TEST INFRASTRUCTURE ONLY: the LDpred2 Gibbs sweep of include/viprs_hip.h (viprs_state_gibbs_sweep) replayed on the host,
 * one column per call, with the draws handed in.  Built at test time by tests/gibbs_replay.py with -O2 -ffp-contract=off:
 * every operation below is rounded on its own, and the q updates go through libm's fmaf.  The sigmoid is the expression of
 * the oracle's grid column (oracle/estep_oracle_impl.h, e_step.hpp:245-261) with libm's expf; the walk over the rows, the
 * axpy, the symmetric form's diagonal term and the upper form's second pass are those of e_step.hpp:387-442; only the update
 * of one SNP differs. */
#include <math.h>
#include <stdint.h>

static float sigmoid_f32(float x) {
    if (x < 0) {
        float e = expf(x);
        return (float)((double)e / (1. + (double)e));
    } else {
        float e = expf(-x);
        return (float)(1. / (1. + (double)e));
    }
}

#define GIBBS_SWEEP(SUF, U)                                                                                             \
    int gibbs_replay_sweep_##SUF(int64_t m, const int32_t* lb, const int64_t* ip, const U* ld, int low_memory,           \
                                 const float* std_beta, const float* mu_mult, const float* hvt, const float* u_logs,     \
                                 const float* unif, const float* noise, float* eta, float* q, float* eta_diff,           \
                                 float* var_mu, float* var_gamma, float dq) {                                            \
        if (m < 0 || !lb || !ip || !std_beta || !mu_mult || !hvt || !u_logs || !unif || !noise || !eta || !q ||          \
            !eta_diff || !var_mu || !var_gamma)                                                                         \
            return -1;                                                                                                  \
        for (int64_t j = 0; j < m; ++j) {                                                                               \
            const float mu = mu_mult[j] * (std_beta[j] - q[j]);                                                         \
            const float u = u_logs[j] + hvt[j] * mu * mu;                                                               \
            const float gamma = sigmoid_f32(u);                                                                         \
            const float b = gamma > unif[j] ? mu + noise[j] : 0.0f;                                                     \
            const float d = b - eta[j];                                                                                 \
            var_mu[j] = mu;                                                                                             \
            var_gamma[j] = gamma;                                                                                       \
            eta_diff[j] = d;                                                                                            \
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

GIBBS_SWEEP(f32, float)
GIBBS_SWEEP(i8, int8_t)
GIBBS_SWEEP(i16, int16_t)
