// lr_control.hip -- the KL-adaptive step size, kept on the device (no counterpart in the reference).
//
//   L1  init    state = {lr, 0, 0, 0, 0, 0}, lr_out = (float)lr
//   L2  adapt   one update's decision from the eight all-reduced diagnostic sums of its last epoch (uav_set_ppo_diag):
//               kl = S[KL_K3] / S[COUNT]; above 2 desired_kl the rate is divided by `factor`, below desired_kl / 2 multiplied,
//               clamped to [lr_min, lr_max]; lr_out = (float)lr is what uav_clip_adam_dlr reads in the next update.
//
// One thread and six doubles, every line the f64 operation uavppo/lr_control.py (adapt_rule) states in numpy, in its order:
// the state is bit-equal to the host's replay of a run.  Nothing is read by the host between an update's diagnostics and the
// next update's Adam steps; the ranks hold the same all-reduced row and so compute the same rate.
#include "common.h"

__global__ void lr_init_kernel(double* __restrict__ state, double lr, float* __restrict__ lr_out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    state[UAV_LR_STATE_LR] = lr;
    for (int i = 1; i < UAV_LR_STATE_N; ++i) state[i] = 0.0;
    lr_out[0] = (float)lr;
}

__global__ void lr_adapt_kernel(double* __restrict__ state, const double* __restrict__ diag8, double desired_kl, double factor,
                                double lr_min, double lr_max, float* __restrict__ lr_out) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double lr = state[UAV_LR_STATE_LR];
    const double n = diag8[UAV_PPO_DIAG_COUNT];
    double kl = __builtin_nan("");                      // no samples: no estimate (and one NaN pattern, whatever produced it)
    int slot = UAV_LR_STATE_SKIPPED;
    if (n > 0.0) {
        const double q = diag8[UAV_PPO_DIAG_KL_K3] / n;
        if (q == q) {
            kl = q;
            if (q > 2.0 * desired_kl) {
                lr = lr / factor;
                if (lr < lr_min) lr = lr_min;
                slot = UAV_LR_STATE_LOWERED;
            } else if (q < desired_kl / 2.0) {
                lr = lr * factor;
                if (lr > lr_max) lr = lr_max;
                slot = UAV_LR_STATE_RAISED;
            } else {
                slot = UAV_LR_STATE_HELD;
            }
        }
    }
    state[UAV_LR_STATE_LR] = lr;
    state[UAV_LR_STATE_LAST_KL] = kl;
    state[slot] += 1.0;
    lr_out[0] = (float)lr;
}

extern "C" {

int uav_lr_init(uav_ctx* ctx, double* state, double lr, float* lr_out, uav_stream stream) {
    UAV_REQUIRE(ctx && state && lr_out, "uav_lr_init: NULL argument");
    UAV_REQUIRE(lr > 0.0 && lr < (double)__builtin_inff(), "uav_lr_init: lr=%g must be positive and finite", lr);
    hipLaunchKernelGGL(lr_init_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, lr, lr_out);
    UAV_LAUNCH_CHECK();
    return 0;
}

int uav_lr_adapt(uav_ctx* ctx, double* state, const double* diag8, double desired_kl, double factor, double lr_min,
                 double lr_max, float* lr_out, uav_stream stream) {
    UAV_REQUIRE(ctx && state && diag8 && lr_out, "uav_lr_adapt: NULL argument");
    UAV_REQUIRE(desired_kl > 0.0 && desired_kl < (double)__builtin_inff(), "uav_lr_adapt: desired_kl=%g must be positive and finite", desired_kl);
    UAV_REQUIRE(factor > 1.0, "uav_lr_adapt: factor=%g must be greater than 1", factor);
    UAV_REQUIRE(lr_min > 0.0, "uav_lr_adapt: lr_min=%g must be positive", lr_min);
    UAV_REQUIRE(lr_min <= lr_max, "uav_lr_adapt: lr_min=%g is greater than lr_max=%g", lr_min, lr_max);
    hipLaunchKernelGGL(lr_adapt_kernel, dim3(1), dim3(64), 0, as_stream(stream), state, diag8, desired_kl, factor, lr_min,
                       lr_max, lr_out);
    UAV_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
