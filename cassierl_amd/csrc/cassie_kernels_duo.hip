// cassie_kernels_duo.hip -- gfx950 backend and kernel of the 64-environments-per-wavefront Env.step (cassie_duo_core.h): the lane-per-leg
// set-up of cassie_leg_core.h for two groups of 32 environments, one joint PGS sweep with a lane per environment.
//
//   workgroup b (one wavefront), lane 2e + k:  leg k of environment 64 b + e (group A) AND of environment 64 b + 32 + e (group B)
//   in the sweeps:  even lane 2e = environment 64 b + e, odd lane 2e + 1 = environment 64 b + 32 + e  (both legs each)
//
// LDS (39 168 B per wavefront, four wavefronts per CU -- the budget of the two-lanes kernel, now for twice the environments): per group the
// per-lane slots a substep itself produces and consumes (clock, sum of squared actions, smooth force, link origins, two contact-pair
// descriptors); the third pair and the joint-limit descriptors exist once (a group that needs them is solved before the other group's
// set-up begins).  What the two-lanes kernel kept in LDS for the whole step and touched once -- setState snapshot, qstate, motor commands,
// action -- is read from / written to the HBM record and the action row where it is used (`DuoLds::cld / cst` route the slot numbers).
#ifndef CASSIE_KERNELS_DUO_HIP_
#define CASSIE_KERNELS_DUO_HIP_
#include "cassie_kernels_leg.hip"
#include "cassie_duo_core.h"

namespace cassie {
namespace leg {

constexpr int DUO_WAVES = 2;   // independent wavefronts per workgroup (no barrier, no shared data).  A/B r05, 65 536 envs: 1 -> 1.146 ms, 2 -> 1.125, 4 -> 1.129
#define DUO_LANE ((int)threadIdx.x & 63)
constexpr int DUO_PHASES = 24;   // profiling builds: cycle accumulators of this kernel (CASSIE_PHASE_WORDS of cassie_cabi.hip)
__device__ const double duo_zero_action[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // the action row of a step without actions
struct DuoShared {
  double cold[2][20][64];    // per group: clock, a2, tau_b 3, tau_l 5, link origins x 5, z 5 (the pelvis origin is the constant 0)
  double pr[2][2][4][64];    // per group: contact pairs 0, 1
  double pr2[4][64];         // third pair (eight-row path only)
  double lm[4][3][64];       // joint limits (eight-row path only)
  int pdepth[2][2][64];
  int pdepth2[64];
  int lmj[4][64];
};
static_assert(sizeof(DuoShared) == 39168, "LDS budget of four wavefronts per CU");

struct DevDuoB : DevB {
  // sub_setup: a group on its feet does not build its two empty row slots and warm-starts over six.  r05 had this off for this kernel (the branch cost 75 more
  // spills with the eight-row pair solve inline behind the set-up: 1.01 -> 1.08 ms); r06: the eight-row groups leave for the joint sweep like the others, the
  // set-up's two branches end in their own stores to the workspace and never meet again: 304 B of scratch instead of 264, **1.018 -> 0.990 ms** per 65 536-env
  // step (tools/ab_bench.py, both orders), bit-identical.
  static constexpr bool SPLIT_TAIL = true;
  // a row word of group B where the direct path begins (Duo::env_step2): the same bits as a new value, so that its live range starts there and not in the set-up
  static LEG_FN void fresh(double& x) { asm volatile("" : "+v"(x)); }
  // per-wavefront workspace in global memory (Duo::W_*): [slot][lane], the lane's pointer is the base of its column
  // Buffer addressing: one resource descriptor per wavefront (SGPRs), the lane's byte offset in ONE VGPR, the slot as the scalar offset
  // of the instruction -- so a slot costs an s_mov, not a 64-bit per-lane pointer (with plain pointers the compiler materialises one
  // pointer per slot beyond the 4 KB immediate range, ~150 of them, and spills them: first build of this path).
  struct W { __amdgpu_buffer_rsrc_t r; unsigned voff; };
  typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  // slots 2p and 2p + 1 of a lane are adjacent: [p][lane][2] -- a pair of slots is ONE sixteen-byte access per lane (1 KB per wavefront)
  static LEG_FN constexpr int wofs(int slot) { return (slot >> 1) * 1024 + (slot & 1) * 8; }
  static LEG_FN double wld(W ws, int slot) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(ws.r, ws.voff, wofs(slot), 0);
    return __hiloint2double((int)v.y, (int)v.x);
  }
  static LEG_FN void wst(W ws, int slot, double v) {
    u32x2 w; w.x = (unsigned)__double2loint(v); w.y = (unsigned)__double2hiint(v);
    __builtin_amdgcn_raw_buffer_store_b64(w, ws.r, ws.voff, wofs(slot), 0);
  }
  static LEG_FN void wld2(W ws, int slot, double& a, double& b) {   // slot even
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(ws.r, ws.voff, wofs(slot), 0);
    a = __hiloint2double((int)v.y, (int)v.x); b = __hiloint2double((int)v.w, (int)v.z);
  }
  static LEG_FN void wst2(W ws, int slot, double a, double b) {
    u32x4 w; w.x = (unsigned)__double2loint(a); w.y = (unsigned)__double2hiint(a); w.z = (unsigned)__double2loint(b); w.w = (unsigned)__double2hiint(b);
    __builtin_amdgcn_raw_buffer_store_b128(w, ws.r, ws.voff, wofs(slot), 0);
  }
  // The batch arrays (state records, action / observation rows, reward, done flags) are addressed the same way: `P` is ONE descriptor over the whole
  // array (wave-uniform, built from the kernel arguments where a phase needs it: scalar registers) and the byte offset of the lane's row in one
  // VGPR.  An access costs no 64-bit per-lane pointer -- six of them per group were what the allocator spilled, and every store behind a spilled
  // pointer waited for the pointer's reload, i.e. for every store before it (vmcnt counts stores until they are acknowledged).  num_records is the
  // array's size in bytes: the hardware drops a store (and zeroes a load) beyond it.
  struct P { __amdgpu_buffer_rsrc_t r; unsigned voff; };
  typedef P P8;
  static LEG_FN double pld(P p, int off) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(p.r, p.voff + (unsigned)off * 8u, 0, 0);
    return __hiloint2double((int)v.y, (int)v.x);
  }
  static LEG_FN void pst(P p, int off, double v, bool m) {
    if (m) {
      u32x2 w; w.x = (unsigned)__double2loint(v); w.y = (unsigned)__double2hiint(v);
      __builtin_amdgcn_raw_buffer_store_b64(w, p.r, p.voff + (unsigned)off * 8u, 0, 0);
    }
  }
  static LEG_FN void pst8(P8 p, bool v, bool m) { if (m) __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, p.r, p.voff, 0, 0); }
#ifdef DUO_VIEW_EXPERIMENT
  // the view of joint lane 2e + k on column 2e + X of group k's block (group stride in slots; see joint_solve_view)
  static LEG_FN W wview(W ws, int group_slots, int X) {
    W v; v.r = ws.r;
    const unsigned lane = ws.voff >> 4;
    v.voff = ((lane & ~1u) + (unsigned)X) * 16u + (lane & 1u) * (unsigned)(group_slots / 2) * 1024u;
    return v;
  }
  template <int N> static LEG_FN void wput_if(W ws, int first, double (&t)[N], bool m) {
    if (m) { for (int i = 0; i < N; i++) wst(ws, first + i, t[i]); }
  }
  static LEG_FN void wst_if(W ws, int slot, double v, bool m) { if (m) wst(ws, slot, v); }
#endif
  struct Lds {
    DuoShared* sh;
    int g;
    // the group's state record and action row (without actions: the zero row); recl / recm / actl: the same with the lane's leg offset (lo doubles: joints,
    // ao doubles: motors) folded into the lane offset where the group is selected, so that a slot number is the instruction's immediate offset (added to
    // `lo` first it is a loop-invariant per-lane value the compiler hoists out of the substep loop and parks, one register per slot)
    P rec, recl, recm, actl;
    bool snap;
    int lo, ao;
#ifdef CASSIE_PHASE_TIMING   // profiling builds (tools/phase_profile.py duo): shader cycles per phase of this wavefront; the time up to mark(k) goes to bucket k
    unsigned long long t_last, acc[DUO_PHASES];   // 16..21: the pieces of the glue (records in, bookkeeping, outputs, write-back), buckets of their own
    bool rp = false;   // the pass that is running is the reset pass (env_step2)
    LEG_FN void in_reset_pass(bool on) { rp = on; }
    LEG_FN void mark(int k) {
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      const unsigned long long n = __builtin_readcyclecounter();
#ifdef CASSIE_PHASE_RESET_ONLY   // the buckets of the reset pass alone (tools/phase_profile_duo.py); bucket 0 = its glue (with two outputs calls -- terrain -- the second call too)
      if (rp)
#endif
      acc[k < DUO_PHASES ? k : 0] += n - t_last;
      t_last = n;
      __builtin_amdgcn_sched_barrier(0);
    }
#else
    LEG_FN void mark(int) {}
#endif
    template <class IoT> LEG_FN void select(int group, const IoT& io) { 
      g = group; rec = io.rec; recl = io.rec; recm = io.rec; actl = io.act;
      recl.voff += (unsigned)lo * 8u; recm.voff += (unsigned)ao * 8u; actl.voff += (unsigned)ao * 8u;
    }
    LEG_FN void snapshot(bool on) { snap = on; }
    // slot of the group's cold block, or -1: not in LDS
    static LEG_FN constexpr int slot(int i) {
      return i == 24 ? 0 : i == 28 ? 1 : (i >= 29 && i < 37) ? i - 27 : (i >= 38 && i < 43) ? i - 28 : (i >= 44 && i < 49) ? i - 29 : -1;
    }
    LEG_FN double cld(int i) const {
      const int l = DUO_LANE;
      if (i < 8) return i < 3 ? pld(rec, ES_KQ + i) : pld(recl, ES_KQ + (i - 3));
      if (i < 16) return i - 8 < 3 ? pld(rec, ES_KV + (i - 8)) : pld(recl, ES_KV + (i - 11));
      if (i < 21) return pld(recl, ES_QSTATE + (i - 16));
      if (i < 24) return pld(recm, ES_CTRL + (i - 21));
      if (i >= 25 && i < 28) return pld(actl, i - 25);   // (one unconditional load: three of them go out in one batch)
      if (i == 37 || i == 43) return 0.0;   // origin of the pelvis link relative to the pelvis origin
      return sh->cold[g][slot(i)][l];
    }
    LEG_FN void cst(int i, double v, bool m) {
      const int l = DUO_LANE;
      if (i < 16) {
        const int k = i < 8 ? i : i - 8, f = i < 8 ? ES_KQ : ES_KV;
        if (k < 3) pst(rec, f + k, v, snap && m); else pst(recl, f + (k - 3), v, snap && m);
      } else if (i < 21) pst(recl, ES_QSTATE + (i - 16), v, m);
      else if (i < 24) pst(recm, ES_CTRL + (i - 21), v, m);
      else if (i >= 25 && i < 28) {}
      else if (i == 37 || i == 43) {}
      else { if (m) sh->cold[g][slot(i)][l] = v; }
    }
    LEG_FN void st_pair(int s, double px, double pz, double dist, double invw, int depth, bool m) {
      if (m) {
        const int l = DUO_LANE;
        double* p = s < 2 ? &sh->pr[g][s][0][l] : &sh->pr2[0][l];
        p[0] = px; p[64] = pz; p[128] = dist; p[192] = invw;
        *(s < 2 ? &sh->pdepth[g][s][l] : &sh->pdepth2[l]) = depth;
      }
    }
    LEG_FN void ld_pair(int s, double& px, double& pz, double& dist, double& invw, int& depth) const {
      const int l = DUO_LANE;
      if (s < 2) { px = sh->pr[g][s][0][l]; pz = sh->pr[g][s][1][l]; dist = sh->pr[g][s][2][l]; invw = sh->pr[g][s][3][l]; depth = sh->pdepth[g][s][l]; }
      else { px = sh->pr2[0][l]; pz = sh->pr2[1][l]; dist = sh->pr2[2][l]; invw = sh->pr2[3][l]; depth = sh->pdepth2[l]; }
    }
    LEG_FN void st_lim(int slot_, double pos, double sgn, double invw, int j, bool m) {
      if (m) {
        const int l = DUO_LANE;
        sh->lm[slot_][0][l] = pos; sh->lm[slot_][1][l] = sgn; sh->lm[slot_][2][l] = invw; sh->lmj[slot_][l] = j;
      }
    }
    LEG_FN void ld_lim(int s, double& pos, double& sgn, double& invw, int& j) const {
      const int l = DUO_LANE;
      pos = sh->lm[s][0][l]; sgn = sh->lm[s][1][l]; invw = sh->lm[s][2][l]; j = sh->lmj[s][l];
    }
  };
};

typedef Duo<DevDuoB> DDuo;
static_assert(DDuo::C::C_TIME == 24 && DDuo::C::C_A2 == 28 && DDuo::C::C_TAUB == 29 && DDuo::C::C_OX == 37 && DDuo::C::C_OZ == 43 && DDuo::C::C_N == 49 &&
              DDuo::C::C_KQ == 0 && DDuo::C::C_KV == 8 && DDuo::C::C_QST == 16 && DDuo::C::C_CTRL == 21 && DDuo::C::C_ACT == 25, "DuoLds routes these slot numbers");

// The group's rows of the batch arrays (env_io of cassie_kernels_leg.hip for this backend's P): descriptors over the launch's n_envs rows, lane offsets
// of environment `env`.  A lane past the batch addresses row 0 (its stores are masked by the caller, as they always were); an array the launch does not
// have is a descriptor of no bytes; a launch without actions reads the zero row.  32-bit byte offsets: the host keeps a batch whose records exceed 4 GiB out of this tier.
template <class Io> LEG_FN Io duo_io(const VecParams& p, int env, bool want_obs) {
  const unsigned n = (unsigned)p.n_envs, e = (unsigned)DevB::opq(env < p.n_envs ? env : 0);
  auto rows = [](const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);   // (word 3: 32-bit data format, gfx9 encoding)
  };
  Io io;
  io.has_act = p.actions != nullptr;
  io.has_tobs = p.terminal_obs != nullptr;
  const unsigned arow = io.has_act ? (unsigned)p.adim * 8u : 0u;
  io.rec.r = rows(p.state, n * (unsigned)(ENV_STRIDE * 8)); io.rec.voff = e * (unsigned)(ENV_STRIDE * 8);
  io.act.r = rows(io.has_act ? p.actions : duo_zero_action, io.has_act ? n * arow : (unsigned)sizeof(duo_zero_action)); io.act.voff = e * arow;
  io.obs.r = rows(p.obs, want_obs ? n * 208u : 0u); io.obs.voff = want_obs ? e * 208u : 0u;
  io.tobs.r = rows(p.terminal_obs, io.has_tobs ? n * 208u : 0u); io.tobs.voff = io.has_tobs ? e * 208u : 0u;
  io.rew.r = rows(p.reward, want_obs ? n * 8u : 0u); io.rew.voff = want_obs ? e * 8u : 0u;
  io.done.r = rows(p.done, want_obs ? n : 0u); io.done.voff = want_obs ? e : 0u;
  return io;
}

constexpr size_t duo_workspace_doubles_per_wave = (size_t)DDuo::W_N * 64;
// THE WORKSPACE IS A PROPERTY OF THE CHIP, NOT OF THE BATCH (r06).  One wavefront of this kernel owns a SIMD (512 registers), so at most
// 4 x CUs wavefronts exist at any time, however many the launch has.  A batch of up to DuoSlots::DIRECT_MAX tasks (one round of an MI355X,
// the headline's 65 536 envs) indexes the workspace by its task number, as r05 did.  A larger batch CLAIMS a slot per wavefront from a table
// of `mask + 1` busy words (a power of two >= 2 x the chip's SIMDs, one eighth of it per XCD): the first probe is a hash of the wavefront's physical place
// (XCC, SE, CU, SIMD from HW_REG_XCC_ID / HW_REG_HW_ID) -- two resident wavefronts of this kernel cannot share a SIMD, so the probe finds its
// word free and the same SIMD comes back to the same 176 KB (of which a batch on its feet touches 139), launch after launch: 180 MB touched on an MI355X for any batch (360 MB allocated: two words per SIMD), Infinity-Cache
// resident (r05 indexed by the task: 1.14 GB at 524 288 envs).  The place is only a HINT: the claim is an atomic compare-and-swap with linear
// probing, so a collision (another hash layout, a future part, the test mode that zeroes the hint) costs probes (STAT_WS_PROBES), never a
// result.  The hardware's dispatcher stays the task queue: a wavefront that lost the arbitration for the fabric (-7..+10 % lifetime spread,
// profiles/r05_phase_duo.txt) simply frees its SIMD later, and the next workgroup goes where a SIMD is free.
// (Built and measured first as a persistent grid pulling tasks from a counter: the task loop around the body cost 68 B more scratch per lane
// and +1.5 % at every batch size, profiles/r06_size_sweep.jsonl.)
struct DuoSlots {
  static constexpr int DIRECT_MAX = 1024;   // tasks up to which the workspace is indexed by the task (host: cassie_cabi.hip sizes it)
  unsigned* busy;      // null: slot = task
  unsigned mask;       // table size - 1
  unsigned flat_hint;  // tests: every wavefront starts probing at word 0
  __device__ __forceinline__ int claim(int lane, int task, unsigned long long* stats) const {
    if (!busy) return task;
    unsigned h = 0;
    if (lane == 0) {
      // HW_REG_HW_ID (4): WAVE_ID [3:0], SIMD_ID [5:4], PIPE_ID [7:6], CU_ID [11:8], SH_ID [12], SE_ID [15:13]; HW_REG_XCC_ID (20): XCC_ID [3:0]
      // (s_getreg operand: size - 1 << 11 | offset << 6 | register).  MI355X census (profiles/tools/hwid_census.hip, profiles/r06_hwid_census.txt):
      // XCC 0..7, SE 0..3, SH 0, CU 0..8, SIMD 0..3 -- 1152 places, 1024 of them active; key = xcc:3 | se:2 | cu:4 | simd:2 is injective there
      // (2048 words).  Bits a larger part might use (SE bit 2, SH, XCC bit 3) are folded in: they can only cost probes.
      const unsigned hw = __builtin_amdgcn_s_getreg((32 - 1) << 11 | 0 << 6 | 4);
      const unsigned xcc = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 0 << 6 | 20);
      const unsigned simd = (hw >> 4) & 3u, cu = (hw >> 8) & 15u, sh = (hw >> 12) & 1u, se = (hw >> 13) & 7u;
      // The table is PARTITIONED BY XCD (xcc in the top three bits of the word index, probing wraps inside the partition): a slot is only ever
      // re-used by wavefronts of one XCD, i.e. through one L2 -- the per-XCD L2s are not coherent with each other inside a launch, and a slot
      // that moved between XCDs would need its old owner's dirty lines written back first (an agent-scope release = buffer_wbl2 of the whole
      // L2: measured, 5 % of the launch at 131 072 envs).
      const unsigned part = (mask + 1u) >> 3, pm = part - 1u;
      const unsigned base = (xcc & 7u) * part;
      unsigned k = flat_hint ? 0u : ((se & 3u) << 6 | cu << 2 | simd) + 37u * (sh + 2u * (se >> 2) + 4u * (xcc >> 3));
      unsigned probes = 0;
      while (atomicCAS(busy + base + (k & pm), 0u, 1u) != 0u) { k++; probes++; }
      h = base + (k & pm);
      if (probes && stats) atomicAdd(stats + STAT_WS_PROBES, (unsigned long long)probes);
    }
    return __builtin_amdgcn_readfirstlane((int)h);
  }
  __device__ __forceinline__ void release(int lane, int slot) const {
    // every store of this task to the workspace has reached the L2 (vmcnt counts stores until they are acknowledged) before the word is freed;
    // the next owner is a wavefront of the same XCD (see claim), so no write-back of the L2 is needed: a relaxed store
    if (busy) {
      __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt 6:4 and lgkmcnt 11:8 left at their maxima)
      if (lane == 0) __hip_atomic_store(busy + slot, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
};

inline DuoSlots duo_slots_of(double* workspace, int table_slots, bool flat_hint) {   // host: the launch's claim table (none up to DIRECT_MAX tasks)
  DuoSlots sl;
  sl.busy = table_slots ? reinterpret_cast<unsigned*>(workspace + (size_t)table_slots * duo_workspace_doubles_per_wave) : nullptr;
  sl.mask = table_slots ? (unsigned)table_slots - 1u : 0u;
  sl.flat_hint = flat_hint ? 1u : 0u;
  return sl;
}

// MODE: 0 PD, 1 torque, 2 motor commands from the state record.  pending[env] as env_step_leg_kernel.  workspace: W_N slots x 64 lanes per
// wavefront SLOT (launch::duo_workspace_bytes; contents only live inside one task of one launch).
template <int MODE>
__global__ void __launch_bounds__(64 * DUO_WAVES, 1) env_step_duo_kernel(VecParams p, int* pending, double* workspace, DuoSlots sl) {
  __shared__ DuoShared shs[DUO_WAVES];
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // wave-uniform: LDS addressing stays on a scalar base
  DuoShared& sh = shs[wv];
  const int lane = threadIdx.x & 63;
  const int wave_id = blockIdx.x * DUO_WAVES + wv;
  const EnvCfg cfg = env_cfg(p);
  bool valid[2];
  size_t e[2];
#pragma unroll
  for (int g = 0; g < 2; g++) {
    const int env = wave_id * 64 + g * 32 + (lane >> 1);
    valid[g] = env < p.n_envs;
    e[g] = valid[g] ? (size_t)env : 0;
  }
  // the group's descriptors and lane offsets, rebuilt where a phase needs them
  auto io_of = [&](int g) {
    const int env = wave_id * 64 + g * 32 + (lane >> 1);
    return duo_io<DDuo::Io>(p, env, cfg.want_obs);
  };
  DevDuoB::Lds lds;
  lds.sh = &sh; lds.g = 0; lds.snap = true;   // (rec / act: Lds::select, before any access)
  lds.lo = (lane & 1) * 5 + 3; lds.ao = (lane & 1) * 3;
  DDuo::Out o[2];
  DevDuoB::W ws;   // raw buffer over this wavefront's W_N x 512 bytes (word 3: 32-bit data format, gfx9 encoding)
  const int slot = sl.claim(lane, wave_id, p.stats);
  ws.r = __builtin_amdgcn_make_buffer_rsrc(workspace + (size_t)slot * duo_workspace_doubles_per_wave, 0, DDuo::W_N * 512, 0x00020000);
  ws.voff = (unsigned)lane * 16u;
#ifdef CASSIE_PHASE_TIMING
  for (int i = 0; i < DUO_PHASES; i++) lds.acc[i] = 0;
  lds.t_last = __builtin_readcyclecounter();
#endif
  DDuo::env_step2<MODE>(cfg, lds, ws, io_of, valid, o);
  sl.release(lane, slot);   // (the write-back at the end of env_step2 has consumed its loads from the workspace: they fed its stores to the records)
#ifdef CASSIE_PHASE_TIMING
  lds.mark(0);
  if (lane == 0 && p.phase) for (int i = 0; i < DUO_PHASES; i++) atomicAdd(p.phase + i, lds.acc[i]);
#endif
#pragma unroll
  for (int g = 0; g < 2; g++)
    if (valid[g] && (lane & 1) == 0) report(p, pending, e[g], o[g].pend, o[g].bad);
}

#ifdef CASSIE_LEG_HF
// ---------------------------------------------------------------- height-field instantiation (tu_duo_hf.hip)
// One more per-lane word per contact pair (the x component of the local terrain normal).  LDS stays at four wavefronts per CU: pair 0's normal
// takes the slot of the sum of squared actions (which this backend keeps in two registers instead), pair 1's and the third pair's get three new
// slots: 39 168 + 1536 = 40 704 B.
struct DuoSharedHF : DuoShared {
  double nrm1[2][64];
  double nrm2[64];
};
static_assert(sizeof(DuoSharedHF) == 40704, "LDS budget of four wavefronts per CU");

struct DevDuoBHF : DevDuoB {
  struct Lds : DevDuoB::Lds {
    DuoSharedHF* shf;
    double a2[2];
    // the batch's terrain library: ids of this wavefront's 64 environments (from fid0) and how many of them exist -- wave-uniform, so
    // scalar registers; the set-up serves two groups per lane, so the environment is the GROUP's (g), not the lane's
    const int* fid0;
    int fid_n, n_fields;
    LEG_FN const Terrain& terrain(const Terrain* lib) const {
      const int e = g * 32 + (DUO_LANE >> 1);
      return terrain_of(lib, fid0, n_fields, e < fid_n ? e : 0);
    }
    LEG_FN double cld(int i) const { return i == 28 ? (g == 0 ? a2[0] : a2[1]) : DevDuoB::Lds::cld(i); }
    LEG_FN void cst(int i, double v, bool m) {
      if (i == 28) { if (m) { if (g == 0) a2[0] = v; else a2[1] = v; } }
      else DevDuoB::Lds::cst(i, v, m);
    }
    LEG_FN void st_nrm(int slot, double nx, bool m) {
      if (m) { const int l = DUO_LANE; *(slot == 0 ? &shf->cold[g][1][l] : slot == 1 ? &shf->nrm1[g][l] : &shf->nrm2[l]) = nx; }
    }
    LEG_FN double ld_nrm(int s) const { const int l = DUO_LANE; return s == 0 ? shf->cold[g][1][l] : s == 1 ? shf->nrm1[g][l] : shf->nrm2[l]; }
  };
  static LEG_FN void hf_sphere(const Terrain& t, double wx, double wy, double wz, double radius, double& dist, double& nx, double& nz) {
    cassie::terrain_sphere(t, wx, wy, wz, radius, dist, nx, nz);
  }
};
typedef Duo<DevDuoBHF> DDuoHF;
static_assert(DDuoHF::W_N == DDuo::W_N, "one workspace size for both instantiations");

template <int MODE>
__global__ void __launch_bounds__(64 * DUO_WAVES, 1) env_step_duo_hf_kernel(VecParams p, int* pending, double* workspace, DuoSlots sl) {
  __shared__ DuoSharedHF shs[DUO_WAVES];
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  DuoSharedHF& sh = shs[wv];
  const int lane = threadIdx.x & 63;
  const int wave_id = blockIdx.x * DUO_WAVES + wv;
  const EnvCfg cfg = env_cfg(p);
  bool valid[2];
  size_t e[2];
#pragma unroll
  for (int g = 0; g < 2; g++) {
    const int env = wave_id * 64 + g * 32 + (lane >> 1);
    valid[g] = env < p.n_envs;
    e[g] = valid[g] ? (size_t)env : 0;
  }
  auto io_of = [&](int g) {
    const int env = wave_id * 64 + g * 32 + (lane >> 1);
    return duo_io<DDuoHF::Io>(p, env, cfg.want_obs);
  };
  DevDuoBHF::Lds lds;
  lds.sh = &sh; lds.shf = &sh; lds.g = 0; lds.snap = true;   // (rec / act: Lds::select, before any access)
  lds.lo = (lane & 1) * 5 + 3; lds.ao = (lane & 1) * 3;
  lds.a2[0] = 0.0; lds.a2[1] = 0.0;
  {
    const int w0 = wave_id * 64 < p.n_envs ? wave_id * 64 : 0;   // (a wavefront past the batch sets nothing up; its index stays in the array all the same)
    lds.fid0 = p.hf.ids + w0; lds.fid_n = p.n_envs - w0; lds.n_fields = p.hf.n_fields;
  }
  DevDuoBHF::W ws;
  const int slot = sl.claim(lane, wave_id, p.stats);   // (as env_step_duo_kernel)
  ws.r = __builtin_amdgcn_make_buffer_rsrc(workspace + (size_t)slot * duo_workspace_doubles_per_wave, 0, DDuoHF::W_N * 512, 0x00020000);
  ws.voff = (unsigned)lane * 16u;
  DDuoHF::Out o[2];
  DDuoHF::env_step2<MODE, true>(cfg, lds, ws, io_of, valid, o, p.hf.fields);
  sl.release(lane, slot);
#pragma unroll
  for (int g = 0; g < 2; g++)
    if (valid[g] && (lane & 1) == 0) report(p, pending, e[g], o[g].pend, o[g].bad);
}
#else
template <int MODE> __global__ void env_step_duo_hf_kernel(VecParams p, int* pending, double* workspace, DuoSlots sl);   // (declared for step_duo_tier<true>: tu_duo_hf.hip)
#endif

}  // namespace leg

namespace launch {
template <bool HF> void step_duo_tier(int mode, int n_envs, hipStream_t s, const VecParams& p, int* pending, double* workspace, int table_slots, bool flat_hint) {
  const leg::DuoSlots sl = leg::duo_slots_of(workspace, table_slots, flat_hint);
  const int waves = (n_envs + 63) / 64;
  dim3 grid((waves + leg::DUO_WAVES - 1) / leg::DUO_WAVES), block(64 * leg::DUO_WAVES);
  by_mode(mode, [&](auto m) {
    if constexpr (HF) hipLaunchKernelGGL((leg::env_step_duo_hf_kernel<m>), grid, block, 0, s, p, pending, workspace, sl);
    else hipLaunchKernelGGL((leg::env_step_duo_kernel<m>), grid, block, 0, s, p, pending, workspace, sl);
  });
}
}  // namespace launch
}  // namespace cassie
#endif
