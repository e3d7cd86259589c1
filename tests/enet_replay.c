/* TEST INFRASTRUCTURE ONLY: the elastic-net sweep of include/viprs_hip.h (viprs_state_enet_sweep) replayed on the host,
 * one column per call.  Built at test time by tests/enet_replay.py with -O2 -ffp-contract=off: every operation below is
 * rounded on its own, and the q updates go through libm's fmaf -- one rounding, which a float64 emulation does not give.
 * The walk over the rows, the axpy, the symmetric form's diagonal term and the upper form's second pass are those of
 * oracle/estep_oracle_impl.h (e_step.hpp:387-442); only the update of one SNP differs. */
#include <math.h>
#include <stdint.h>

#define ENET_SWEEP(SUF, U)                                                                                              \
    int enet_replay_sweep_##SUF(int64_t m, const int32_t* lb, const int64_t* ip, const U* ld, int low_memory,            \
                                const float* std_beta, const float* c, const float* pen, float* eta, float* q,           \
                                float* eta_diff, float* var_mu, float* var_gamma, float dq) {                            \
        if (m < 0 || !lb || !ip || !std_beta || !c || !pen || !eta || !q || !eta_diff || !var_mu || !var_gamma) return -1; \
        for (int64_t j = 0; j < m; ++j) {                                                                               \
            const float t = c[j] * q[j];                                                                                \
            const float u = std_beta[j] - t;                                                                            \
            const float a = fabsf(u) - pen[j];                                                                          \
            const float b = a > 0.0f ? copysignf(a, u) : 0.0f;                                                          \
            const float d = b - eta[j];                                                                                 \
            var_mu[j] = u;                                                                                              \
            var_gamma[j] = b != 0.0f ? 1.0f : 0.0f;                                                                     \
            eta_diff[j] = d;                                                                                            \
            const float alpha = dq * d;                                                                                 \
            float* x = q + lb[j];                                                                                       \
            const U* y = ld + ip[j];                                                                                    \
            const int64_t len = ip[j + 1] - ip[j];                                                                      \
            for (int64_t i = 0; i < len; ++i) x[i] = fmaf((float)y[i], alpha, x[i]);                                    \
            if (!low_memory) q[j] -= d;                                                                                 \
            eta[j] = eta[j] + d;                                                                                        \
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

ENET_SWEEP(f32, float)
ENET_SWEEP(i8, int8_t)
ENET_SWEEP(i16, int16_t)
