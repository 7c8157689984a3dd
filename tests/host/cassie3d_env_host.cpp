// cassie3d_env_host.cpp -- TEST HARNESS: the arithmetic of the Cassie3d environment layer (cassierl_amd/csrc/cassie3d_env.h: observation,
// reward, done, failure guard) compiled for the CPU.  tests/test_cassie3d_env_cpu.py builds it with g++ into a temporary directory, twice:
//   * as a shared library (env3d_host_finish through ctypes);
//   * with -DENV3D_HOST_MAIN as a stand-alone program, instrumented with -fsanitize=address,undefined, which reads
//       n, then n records of 80 doubles and n action rows of 10 doubles        (binary file, native doubles; n as a double)
//     and writes per environment 45 observation doubles, the reward, done and guard (as doubles) to the output file.
// The product has no CPU path.
#define __device__
#define __constant__
#define __forceinline__ inline
#define C3ENV_FN inline
#include <cmath>
using std::fabs; using std::sqrt; using std::sin; using std::cos;
#include "../../cassierl_amd/csrc/cassie3d_env.h"

extern "C" int env3d_host_finish(const double* recs, const double* actions, int n, double* obs, double* reward, double* done, double* guard) {
  for (int e = 0; e < n; e++) {
    cassie3d::env::StepOut o;
    cassie3d::env::finish(recs + (size_t)e * cassie3d::ENV3_STRIDE, actions + (size_t)e * cassie3d::NU, o);
    for (int i = 0; i < cassie3d::env::NOBS; i++) obs[(size_t)e * cassie3d::env::NOBS + i] = o.obs[i];
    reward[e] = o.reward; done[e] = o.done ? 1.0 : 0.0; guard[e] = o.guard ? 1.0 : 0.0;
  }
  return 0;
}

#ifdef ENV3D_HOST_MAIN
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s <input> <output>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  double nd = 0.0;
  if (fread(&nd, sizeof nd, 1, f) != 1 || !(nd >= 1.0 && nd <= 1e6)) { fprintf(stderr, "bad header\n"); fclose(f); return 2; }
  const size_t n = (size_t)nd;
  std::vector<double> recs(n * cassie3d::ENV3_STRIDE), act(n * cassie3d::NU);
  const bool ok = fread(recs.data(), sizeof(double), recs.size(), f) == recs.size() && fread(act.data(), sizeof(double), act.size(), f) == act.size();
  fclose(f);
  if (!ok) { fprintf(stderr, "short input\n"); return 2; }
  std::vector<double> obs(n * cassie3d::env::NOBS), rew(n), done(n), guard(n);
  env3d_host_finish(recs.data(), act.data(), (int)n, obs.data(), rew.data(), done.data(), guard.data());
  FILE* g = fopen(argv[2], "wb");
  if (!g) { perror(argv[2]); return 2; }
  const bool wrote = fwrite(obs.data(), sizeof(double), obs.size(), g) == obs.size() && fwrite(rew.data(), sizeof(double), n, g) == n &&
                     fwrite(done.data(), sizeof(double), n, g) == n && fwrite(guard.data(), sizeof(double), n, g) == n;
  return fclose(g) == 0 && wrote ? 0 : 2;
}
#endif
