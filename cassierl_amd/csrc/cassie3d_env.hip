// cassie3d_env.hip -- the finish and reset kernels of the Cassie3d environment layer (cassie3d_env.h holds the arithmetic).
//
// One thread per environment, 256 per workgroup.  The finish kernel runs on the handle's stream behind the physics tiers of the step
// (launch3d has joined its side streams by then): it reads the record the step ended in, writes observation, reward, done and -- optionally
// -- the terminal observation, and with auto-reset replaces the whole record of a done environment by the RESET RECORD: what
// Cassie3dVecReset(h, NULL, NULL) leaves (standing pose, time 0, mj_forward's warm start), copied from environment 0 at create.  A reset
// therefore needs no physics launch.  The traffic is the records (640 B per environment, read once) and the outputs: ~17 MB at 16 384
// environments, microseconds beside the physics.
#ifndef CASSIE3D_ENV_HIP_
#define CASSIE3D_ENV_HIP_
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cassie3d_env.h"
#include "cassie_launch.h"

namespace cassie3d {

constexpr int ENV_BLOCK = 256;

// counts the lanes of the wavefront with `flag` set into *counter with one atomic (every lane of the wavefront must call it)
__device__ __forceinline__ void wave_count(bool flag, unsigned long long* counter) {
  const unsigned long long m = __ballot(flag);
  if (m != 0ull && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(counter, (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(ENV_BLOCK) env_finish3d_kernel(EnvFinish3 p) {
  const int e = blockIdx.x * ENV_BLOCK + threadIdx.x;
  const bool valid = e < p.n_envs;
  env::StepOut o;
  o.done = false; o.guard = false;
  if (valid) {
    double* rec = p.state + (size_t)e * ENV3_STRIDE;
    env::finish(rec, p.actions + (size_t)e * NU, o);
    if (p.terminal_obs)
      for (int i = 0; i < env::NOBS; i++) p.terminal_obs[(size_t)e * env::NOBS + i] = o.obs[i];
    if (o.done && p.auto_reset) {
      for (int i = 0; i < ENV3_STRIDE; i++) rec[i] = p.reset_rec[i];
      env::observe(p.reset_rec, o.obs);
    }
    for (int i = 0; i < env::NOBS; i++) p.obs[(size_t)e * env::NOBS + i] = o.obs[i];
    p.reward[e] = o.reward;
    p.done[e] = o.done ? 1 : 0;
  }
  wave_count(o.done, p.counters + ENVC_DONE);
  wave_count(o.guard, p.counters + ENVC_GUARD);
}

// mask == null: every environment.  obs (optional): the observation of EVERY environment after the reset (zeros under the guard).
__global__ void __launch_bounds__(ENV_BLOCK) env_reset3d_kernel(double* state, const uint8_t* mask, const double* reset_rec, double* obs, int n_envs) {
  const int e = blockIdx.x * ENV_BLOCK + threadIdx.x;
  if (e >= n_envs) return;
  double* rec = state + (size_t)e * ENV3_STRIDE;
  if (!mask || mask[e])
    for (int i = 0; i < ENV3_STRIDE; i++) rec[i] = reset_rec[i];
  if (obs) {
    double o[env::NOBS];
    if (env::state_bad(rec)) for (int i = 0; i < env::NOBS; i++) o[i] = 0.0;
    else env::observe(rec, o);
    for (int i = 0; i < env::NOBS; i++) obs[(size_t)e * env::NOBS + i] = o[i];
  }
}

namespace launch {
void env_finish3d(hipStream_t s, const EnvFinish3& p) {
  hipLaunchKernelGGL(env_finish3d_kernel, dim3((p.n_envs + ENV_BLOCK - 1) / ENV_BLOCK), dim3(ENV_BLOCK), 0, s, p);
}
void env_reset3d(int n_envs, hipStream_t s, double* state, const uint8_t* mask, const double* reset_rec, double* obs) {
  hipLaunchKernelGGL(env_reset3d_kernel, dim3((n_envs + ENV_BLOCK - 1) / ENV_BLOCK), dim3(ENV_BLOCK), 0, s, state, mask, reset_rec, obs, n_envs);
}
}  // namespace launch

}  // namespace cassie3d
#endif
