// cassie3d_env.h -- the arithmetic of the Cassie3d ENVIRONMENT layer around the physics: observation, reward, termination and the
// failure guard of one robot from its state record (cassie3d_layout.h).  Plain per-robot code over doubles: one thread per environment
// in the finish kernel (cassie3d_env.hip), and the same source compiled by g++ in the CPU test harness (tests/host/cassie3d_env_host.cpp,
// which defines the HIP qualifiers away, as oracle/leg_host does for the leg cores) -- the library itself has no CPU path.
//
// The reference has no Cassie3d environment (only the MJCF), so the definition is this project's, by analogy to the 2-D standing task
// (rllab/envs/cassie_stand2d.py:118-125) and CassieVecStep (cassie_vec.h):
//   observation [45]  pelvis z | quaternion w x y z | 14 hinge angles | world linear velocity | body-frame angular velocity |
//                     14 hinge rates | left foot - pelvis | right foot - pelvis (world axes)
//                     foot = mean of the leg's *_contact_front and *_contact_rear sites (c3_site_link / c3_site_pos)
//   reward            1 - 2 (0.9 - z)^2 - 2 fx^2 - 2 fy^2 - 0.001 |action|^2,  fx, fy = mean of the two feet's x, y relative to the pelvis
//   done              z < 0.5
//   failure guard     a non-finite qpos / qvel entry or one beyond 1e10 in magnitude: done, reward 0 (cassie_vec.h)
#ifndef CASSIE3D_ENV_H_
#define CASSIE3D_ENV_H_

#include "cassie3d_tables.h"
#include "cassie3d_layout.h"

#ifndef C3ENV_FN
#define C3ENV_FN __device__ __forceinline__
#endif

namespace cassie3d {
namespace env {

constexpr int NOBS = 45;
enum { O_Z = 0, O_QUAT = 1, O_HINGE = 5, O_VLIN = 19, O_VANG = 22, O_RATE = 25, O_FOOT = 39 };
constexpr double Z_TARGET = 0.9, Z_DONE = 0.5, GUARD_MAX = 1e10, ACTION_COST = 0.001;

C3ENV_FN void mv3(const double* m, const double* v, double* r) {
  const double x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2], y = m[3] * v[0] + m[4] * v[1] + m[5] * v[2], z = m[6] * v[0] + m[7] * v[1] + m[8] * v[2];
  r[0] = x; r[1] = y; r[2] = z;
}
C3ENV_FN void mm3(const double* a, const double* b, double* r) {
  double t[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) t[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
  for (int i = 0; i < 9; i++) r[i] = t[i];
}

// Frame of link `link` relative to the pelvis ORIGIN in world axes (pos, mat), by mj_kinematics along c3_link_parent / pos / rot and
// the hinge axes.  The links of a chain are numbered parent before child, at most 15 of them: the path from the pelvis down to the link is
// packed four bits per link, so that no array is indexed at run time.  The hinge of link l >= 1 is dof l + 5, its angle qpos[l + 6].
C3ENV_FN void link_frame(const double* q, int link, double* pos, double* mat) {
  double qw = q[3], qx = q[4], qy = q[5], qz = q[6];
  const double n = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw /= n; qx /= n; qy /= n; qz /= n;
  mat[0] = 1 - 2 * (qy * qy + qz * qz); mat[1] = 2 * (qx * qy - qw * qz); mat[2] = 2 * (qx * qz + qw * qy);
  mat[3] = 2 * (qx * qy + qw * qz); mat[4] = 1 - 2 * (qx * qx + qz * qz); mat[5] = 2 * (qy * qz - qw * qx);
  mat[6] = 2 * (qx * qz - qw * qy); mat[7] = 2 * (qy * qz + qw * qx); mat[8] = 1 - 2 * (qx * qx + qy * qy);
  pos[0] = 0.0; pos[1] = 0.0; pos[2] = 0.0;
  unsigned long long path = 0ull;
  int depth = 0;
  for (int l = link; l > 0 && depth < 15; l = c3_link_parent[l]) { path = (path << 4) | (unsigned long long)l; depth++; }
  for (int k = 0; k < depth; k++, path >>= 4) {
    const int l = (int)(path & 15ull), dof = l + 5;
    double r[3], m0[9], ax[3];
    mv3(mat, c3_link_pos[l], r);
    pos[0] += r[0]; pos[1] += r[1]; pos[2] += r[2];
    mm3(mat, &c3_link_rot[l][0][0], m0);
    mv3(m0, c3_dof_axis[dof], ax);
    const double ang = q[c3_dof_qadr[dof]] - c3_dof_ref[dof], s = sin(ang), c = cos(ang), t1 = 1 - c;   // Rodrigues, applied on the left
    const double R[9] = {c + ax[0] * ax[0] * t1, ax[0] * ax[1] * t1 - ax[2] * s, ax[0] * ax[2] * t1 + ax[1] * s,
                         ax[1] * ax[0] * t1 + ax[2] * s, c + ax[1] * ax[1] * t1, ax[1] * ax[2] * t1 - ax[0] * s,
                         ax[2] * ax[0] * t1 - ax[1] * s, ax[2] * ax[1] * t1 + ax[0] * s, c + ax[2] * ax[2] * t1};
    mm3(R, m0, mat);
  }
}

// foot[leg][3]: mean of the leg's front and rear contact sites minus the pelvis position, world axes
C3ENV_FN void feet(const double* q, double (&foot)[2][3]) {
  for (int leg = 0; leg < 2; leg++) {
    double pos[3], mat[9], a[3], b[3];
    link_frame(q, c3_site_link[2 * leg], pos, mat);   // both sites of a leg sit on its toe link
    mv3(mat, c3_site_pos[2 * leg], a);
    mv3(mat, c3_site_pos[2 * leg + 1], b);
    for (int i = 0; i < 3; i++) foot[leg][i] = pos[i] + 0.5 * (a[i] + b[i]);
  }
}

C3ENV_FN void observe(const double* rec, double* obs) {
  obs[O_Z] = rec[E3_Q + 2];
  for (int i = 0; i < 18; i++) obs[O_QUAT + i] = rec[E3_Q + 3 + i];   // quaternion and the 14 hinge angles, as in the record
  for (int i = 0; i < NV; i++) obs[O_VLIN + i] = rec[E3_V + i];
  double foot[2][3];
  feet(rec + E3_Q, foot);
  for (int i = 0; i < 3; i++) { obs[O_FOOT + i] = foot[0][i]; obs[O_FOOT + 3 + i] = foot[1][i]; }
}

// `action` is the row the caller passed to the step (joint targets in PD mode, motor commands in torque mode)
C3ENV_FN double reward(const double* obs, const double* action) {
  const double dz = Z_TARGET - obs[O_Z], fx = 0.5 * (obs[O_FOOT] + obs[O_FOOT + 3]), fy = 0.5 * (obs[O_FOOT + 1] + obs[O_FOOT + 4]);
  double a2 = 0.0;
  for (int i = 0; i < NU; i++) a2 += action[i] * action[i];
  return 1.0 - 2.0 * dz * dz - 2.0 * fx * fx - 2.0 * fy * fy - ACTION_COST * a2;
}

C3ENV_FN bool fallen(const double* rec) { return rec[E3_Q + 2] < Z_DONE; }

// the failure guard: NaN fails every comparison, so `!(|x| <= max)` catches NaN, +-inf and anything beyond the bound
C3ENV_FN bool state_bad(const double* rec) {
  bool bad = false;
  for (int i = 0; i < NQ; i++) bad = bad || !(fabs(rec[E3_Q + i]) <= GUARD_MAX);
  for (int i = 0; i < NV; i++) bad = bad || !(fabs(rec[E3_V + i]) <= GUARD_MAX);
  return bad;
}

// One environment after its physics step (rec = the state the step ended in): observation, reward and the two flags.  Under the guard
// the observation is zeros and the reward 0.
struct StepOut { double obs[NOBS], reward; bool done, guard; };
C3ENV_FN void finish(const double* rec, const double* action, StepOut& o) {
  o.guard = state_bad(rec);
  if (o.guard) {
    for (int i = 0; i < NOBS; i++) o.obs[i] = 0.0;
    o.reward = 0.0; o.done = true;
    return;
  }
  observe(rec, o.obs);
  o.reward = reward(o.obs, action);
  o.done = fallen(rec);
}

}  // namespace env
}  // namespace cassie3d
#endif
