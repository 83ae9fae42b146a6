// internal_env.h -- the cross-file functions whose signatures need EnvParams / StopRule (internal.h has the rest): kept apart so
// that files without env code do not pull in the device headers.
#pragma once
#include "internal.h"
#include "env_core.h"
#include "stop_rule_core.h"

int env_params_from_cfg(const uav_ctx* ctx, const uav_env_cfg* cfg, int n_env, EnvParams& P);                        // env.hip
// mlp_rollout.hip: the fused MLP rollout and its greedy forms, called by rollout.hip's entry points
int launch_rollout_mlp(uav_ctx* ctx, void* env_state, int n_env, const uav_env_cfg* cfg, const float* params, int horizon, uint64_t iter,
                       float* cur_obs, float* obs, int32_t* act, float* rew, float* val, float* logp, float* done, uint8_t* flags,
                       float* last_val, const int32_t* forced_act, const double* noise, int32_t* nan_count, float* info, float* heads,
                       bool trend, hipStream_t st);
int launch_greedy_mlp(const EnvParams& P, void* env_state, int n_env, const float* params, int steps, float* cur_obs, uint8_t* active,
                      const double* noise, int32_t* act, float* obs, float* pos, uint8_t* flags, int32_t* nan_count, hipStream_t st);
int launch_greedy_mlp_stop(const EnvParams& P, void* env_state, int n_env, const float* params, int steps, float* cur_obs, uint8_t* active,
                           const double* noise, int32_t* act, float* obs, float* pos, uint8_t* flags, int32_t* nan_count,
                           const StopRule& rule, float* stop_win, int32_t* stop_cnt, float* rule_val, hipStream_t st);
