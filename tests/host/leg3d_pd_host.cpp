// leg3d_pd_host.cpp -- TEST HARNESS: the PD mode of the lane-per-leg Cassie3d physics (cassierl_amd/csrc/cassie3d_leg_core.h,
// Core3::env_step<true>) compiled for the CPU with the lane emulation of oracle/leg_host/lane_types.h, as oracle/leg_host/leg3d_host.cpp does
// for torque mode.  Built by tests/test_cassie3d_env_cpu.py with g++ into a temporary directory; the product has no CPU path.
#define __device__
#define __constant__
#define __forceinline__ inline
#define LEG_FN inline
#define LEG3_SUBSTEP_FN inline
#include "../../cassierl_amd/csrc/cassie3d_leg_core.h"

#include "../../oracle/leg_host/lane_types.h"

namespace {

struct HostB3 : HostOps {
  struct K { const double* p[NL]; };
  static K kbase(VI leg) { K k; LANES k.p[l] = &::c3_legk[0][0] + leg.v[l] * LK3_N; return k; }
  static VD kld(K k, int idx) { VD r; LANES r.v[l] = k.p[l][idx]; return r; }
  struct Lds {   // per-lane slots [slot][lane]
    double a[cassie3d::leg::NSLOT3][NL];
    VD ld(int s) const { VD r; LANES r.v[l] = a[s][l]; return r; }
    void st(int s, VD v, VM m) { LANES if (m.v[l]) a[s][l] = v.v[l]; }
    VD ldv(VI s) const { VD r; LANES { const i64 k = s.v[l]; r.v[l] = a[k >= 0 && k < cassie3d::leg::NSLOT3 ? k : 0][l]; } return r; }
    void stv(VI s, VD v, VM m) { LANES if (m.v[l]) a[s.v[l]][l] = v.v[l]; }
  };
};
typedef cassie3d::leg::Core3<HostB3> HCore3;

}  // namespace

extern "C" {

// n_sub PD substeps of n environments on host arrays laid out like the device ones: state [n][80], targets [n][10], gains = kp[10] kd[10].
// pending[e] = substeps NOT done because the environment left the row capacity (its state is untouched from that substep on).
int leg3d_pd_host_step(double* state, const double* targets, const double* gains, int n, int n_sub, int* pending, int* nrows) {
  constexpr int EPG = NL / 2;
  const int groups = (n + EPG - 1) / EPG;
  for (int g = 0; g < groups; g++) {
    const int e0 = g * EPG;
    static thread_local HostB3::Lds lds;
    for (auto& r : lds.a) LANES r[l] = 7.0;   // (a finite non-zero value shows a read of a slot that was never written as a wrong result)
    HCore3::Io io;
    LANES { const int e = e0 + (l >> 1); io.rec.p[l] = state + (size_t)(e < n ? e : e0) * cassie3d::ENV3_STRIDE; }
    io.has_act = true;
    LANES { const int e = e0 + (l >> 1); io.act.p[l] = const_cast<double*>(targets) + (size_t)(e < n ? e : e0) * cassie3d::NU; }
    io.gains = gains;
    VM valid; LANES valid.v[l] = e0 + (l >> 1) < n ? -1 : 0;
    HCore3::Out o;
    HCore3::env_step<true>(lds, io, valid, n_sub, true, o);
    for (int k = 0; k < EPG && e0 + k < n; k++) {
      if (pending) pending[e0 + k] = (int)o.pend.v[2 * k];
      if (nrows) nrows[e0 + k] = (int)o.nrows.v[2 * k];
    }
  }
  return 0;
}

}  // extern "C"
