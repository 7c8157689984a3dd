/* cassie3d_vec.h -- batched Cassie3d physics (model/cassie3d_stiff.xml) on MI355X, C ABI of libcassie2d.so.
 *
 * BASELINE.json configs[4] / SURVEY.md section 8 row N3.  The reference has NO Cassie3d interface to mirror: it ships the
 * MJCF (model/cassie3d_stiff.xml:60-193, actuators :184-195) and vestigial hooks only (src/xml_parser.h:321-323,
 * include/RobotInterface.h:54, src/DynamicModel.cpp:250-265).  These entry points therefore follow the conventions of
 * include/cassie_vec.h (the batched form of src/Cassie2d/Cassie2d.cpp:15-27): opaque handle, plain pointers and sizes, int
 * error codes (CASSIE_OK ... from cassie_vec.h), device pointers unless the name ends in Host.
 *
 * What one call computes: n_sub MuJoCo steps (mj_step: PGS / elliptic cones / Euler with implicit joint damping, options of
 * cassie3d_stiff.xml:5) of every environment with the given motor commands held constant -- the 3-D counterpart of
 * Cassie2d::Step (src/Cassie2d/Cassie2d.cpp:86-94).  nq = 21 (world position, unit quaternion w x y z, 14 hinge angles in
 * MJCF order), nv = 20 (world linear velocity, body-frame angular velocity, hinge rates), nu = 10 (MJCF actuator order).
 *
 * No CPU path: Cassie3dVecCreate fails with CASSIE_ENODEVICE when no HIP device is present.
 */
#ifndef CASSIE3D_VEC_H_
#define CASSIE3D_VEC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CASSIE3D_NQ 21
#define CASSIE3D_NV 20
#define CASSIE3D_NU 10
/* one environment record in HBM: qpos[21] qvel[20] qacc_warmstart[20] ctrl[10] time niter nefc overflow pad */
#define CASSIE3D_STATE_STRIDE 80
#define CASSIE3D_OFF_QPOS 0
#define CASSIE3D_OFF_QVEL 21
#define CASSIE3D_OFF_WARMSTART 41
#define CASSIE3D_OFF_CTRL 61
#define CASSIE3D_OFF_TIME 71
#define CASSIE3D_OFF_NITER 72
#define CASSIE3D_OFF_NEFC 73
#define CASSIE3D_OFF_OVERFLOW 74 /* number of substeps of this environment in which the 64-row cap left contacts out (see below) */

typedef struct Cassie3dVec Cassie3dVec;

/* Environment switch read at create time (A/B and cross-check, not part of the contract): CASSIE3D_PAIR=1 runs the first pass with
 * two environments per wavefront (csrc/cassie3d_pair.hip) instead of one; same results to rounding, measured slower. */
int Cassie3dVecCreate(Cassie3dVec** out, int n_envs, int device);
void Cassie3dVecFree(Cassie3dVec* h);
const char* Cassie3dVecLastError(const Cassie3dVec* h);
int Cassie3dVecSetStream(Cassie3dVec* h, void* hip_stream);
int Cassie3dVecSynchronize(Cassie3dVec* h);
/* standing pose (qpos_dev == NULL) or the given [n][21] / [n][20] device arrays; then mj_forward (Cassie2d::Reset, :78-82) */
int Cassie3dVecReset(Cassie3dVec* h, const double* qpos_dev, const double* qvel_dev);
/* n_sub mj_steps with torques_dev [n][10] (pre-clamp motor commands, as Cassie2d::Step takes them) */
int Cassie3dVecStep(Cassie3dVec* h, const double* torques_dev, int n_sub);
double* Cassie3dVecStatePtr(Cassie3dVec* h); /* device [n][CASSIE3D_STATE_STRIDE] */
/* Event counters since create / the last reset of the counters (synchronises the stream):
 *   out4[0] env-substeps requested
 *   out4[1] env-substeps the 32-row kernel handed to the 64-row kernel
 *   out4[2] env-substeps in which more than 64 constraint rows were active (the model's maximum is 69: 6 connect + 12 limit rows
 *           + 17 contacts x 3) and the LAST contacts in MuJoCo order were left out for that substep.  The environment keeps
 *           stepping (no frozen environment); record slot CASSIE3D_OFF_OVERFLOW counts the same per environment.
 *   out4[3] env-substeps the lane-per-leg kernel (first tier) handed to the wavefront-per-environment kernels (row capacity of its per-lane LDS slots) */
int Cassie3dVecGetCounters(Cassie3dVec* h, uint64_t* out4);
int Cassie3dVecResetCounters(Cassie3dVec* h);
/* host-pointer conveniences (tests, small batches) */
int Cassie3dVecStepHost(Cassie3dVec* h, const double* torques, int n_sub);
int Cassie3dVecGetStateHost(Cassie3dVec* h, double* state /*[n][80]*/);
int Cassie3dVecSetStateHost(Cassie3dVec* h, const double* state /*[n][80]*/);
int Cassie3dVecDebugForwardHost(Cassie3dVec* h, const double* torques, double* dbg /*[n][CASSIE3D_DEBUG_STRIDE]*/);
#define CASSIE3D_DEBUG_STRIDE 1869
/* average time of `steps` back-to-back Cassie3dVecStep calls, HIP events on the handle's stream */
int Cassie3dVecTimeSteps(Cassie3dVec* h, const double* torques_dev, int n_sub, int steps, float* avg_ms);


/* ---- The environment layer: an RL environment around the physics, with the vocabulary of CassieVecStep (cassie_vec.h).  The reference
 * has no Cassie3d environment, so the task is defined here by analogy to its 2-D standing task (rllab/envs/cassie_stand2d.py:118-125):
 *   observation [CASSIE3D_NOBS]: pelvis z | quaternion w x y z | 14 hinge angles | world linear velocity | body-frame angular velocity |
 *     14 hinge rates | left foot - pelvis | right foot - pelvis (world axes; a foot = the mean of its two contact sites)
 *   reward: 1 - 2 (0.9 - z)^2 - 2 fx^2 - 2 fy^2 - 0.001 |action|^2 (fx, fy: mean of the feet's x, y relative to the pelvis)
 *   done: z < 0.5.  Failure guard: a non-finite qpos / qvel entry or one beyond 1e10: done, reward 0, observation zeros (the reset
 *     observation with auto-reset).  With auto_reset a done environment's whole record is replaced by the one Cassie3dVecReset(h, NULL,
 *     NULL) leaves.
 * CASSIE3D_CTRL_PD: the action row holds targets of the ten actuated hinges; EVERY substep commands kp (target - q) - kd v from the
 * state at its start (Cassie2d::StepPd, Cassie2d.cpp:96-117), clamped and geared like a torque.  Not available on a handle created under
 * CASSIE3D_PAIR=1 (CASSIE_EINVAL). */
#define CASSIE3D_NOBS 45
#define CASSIE3D_CTRL_TORQUE 0
#define CASSIE3D_CTRL_PD 1
typedef struct { int control_mode, n_substeps, auto_reset; double kp[10], kd[10]; } Cassie3dEnvConfig;
/* before the first Cassie3dVecEnvStep; validates (mode, n_substeps >= 1, auto_reset 0 / 1, gains finite and >= 0); synchronises.
 * A handle that was never configured has kp = 10, kd = 5 (Cassie3dVecSubstepPd). */
int Cassie3dVecEnvConfigure(Cassie3dVec* h, const Cassie3dEnvConfig* cfg);
/* raw PD substeps with the configured gains, no environment layer: n_sub mj_steps towards targets_dev [n][10] */
int Cassie3dVecSubstepPd(Cassie3dVec* h, const double* targets_dev, int n_sub);
/* resets the environments with mask_dev[i] != 0 (NULL: all) to the standing pose; obs_dev [n][45] (or NULL) gets EVERY environment's observation */
int Cassie3dVecEnvReset(Cassie3dVec* h, const uint8_t* mask_dev, double* obs_dev);
/* one environment step: n_substeps substeps under actions_dev [n][10], then obs [n][45], reward [n], done [n]; terminal_obs_dev [n][45]
 * (or NULL): the observation of the state the step ended in, before any reset (zeros under the guard) */
int Cassie3dVecEnvStep(Cassie3dVec* h, const double* actions_dev, double* obs_dev, double* reward_dev, uint8_t* done_dev, double* terminal_obs_dev);
/* the same with host pointers, synchronous (tests); terminal_obs may be NULL */
int Cassie3dVecEnvStepHost(Cassie3dVec* h, const double* actions, double* obs, double* reward, uint8_t* done, double* terminal_obs);
/* out2[0] done flags raised since create; out2[1] of those by the failure guard (synchronises the stream) */
int Cassie3dVecEnvGetCounters(Cassie3dVec* h, uint64_t* out2);

#ifdef __cplusplus
}
#endif
#endif
