"""A handle of either batched ABI gives back what it took.  Every resource of CassieVec / Cassie3dVec is a member that releases itself
(cassierl_amd/csrc/cassie_host.h), the lazily allocated ones included; this test creates a handle of each kind at 4096 environments, uses every
lazily allocated piece once, frees it, and after two warm-up cycles repeats that twenty times: the device's free memory must not sink by more than
one handle's state array (4096 x 88 x 8 bytes).

That bound is a condition, not a measurement.  It catches a leaked state, workspace, overflow, observation or per-environment list buffer (each is
at least a few of those per twenty cycles); it does NOT catch a leaked byte array or single word: twenty of those stay below it.  Those are covered
by construction: hipFree / hipHostFree / hipStreamDestroy / hipEventDestroy appear only in the owner types, and a handle has no raw resource member."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4096
STATE_ARRAY_BYTES = N * 88 * 8


def _cycle(traj, t):
    from cassierl_amd.vec_env import CassieVecEnv, LEG_TIER_ON, DUO_TIER_ON
    from cassierl_amd.vec_env3d import Cassie3dVec
    # 2D: the first tier in its 64-environments form with a claim table; on the flat floor the Env.step in segments (the environment of the test)
    env = CassieVecEnv(N, kind="walk", control_mode="PD", n_substeps=10, flags=LEG_TIER_ON | DUO_TIER_ON)
    info = env.tier_info()
    assert info["first_tier"] == "duo" and info["duo_table_slots"] == 64 and info["duo_envs"] == N
    env.set_trajectory(traj["time"], traj["qpos"])
    env.set_trajectory(traj["time"], traj["qpos"])            # replaces the first table
    env.set_terrain_library([t["field"], t["field"] + 0.01])  # heights, descriptors, ids
    env.set_terrain_ids(t["ids"])                             # the word of the range check
    env.step(t["act"], t["bufs"])                             # on terrain: one launch of the 64-environments kernel, workspace claimed from the table
    env.set_terrain_library([])                               # cleared: the flat floor again
    env.qp_iterations()                                       # allocates the statistics
    env.qp_iterations()
    env.debug_substep_host("PD", t["act_host"])               # debug record and debug overflow workspace
    env.step(t["act"], t["bufs"])                             # flat floor: in segments (lists, streams, events of the segments)
    env.synchronize()
    env.close()
    # 3D: a step in segments, a debug forward
    e3 = Cassie3dVec(N)
    e3.step(t["tq3"], n_sub=10)
    e3.debug_forward_host(t["tq3_host"])
    e3.synchronize()
    e3.close()


def test_twenty_create_use_free_cycles_keep_the_free_memory(traj, monkeypatch):
    import torch
    from cassierl_amd.vec_env import action_space
    monkeypatch.setenv("CASSIE2D_DUO_TABLE", "64")
    monkeypatch.setenv("CASSIE2D_SIDE_BY_SIDE", "1")
    monkeypatch.setenv("CASSIE2D_SEGMENTS", "1")
    box = action_space("PD")
    act_host = np.tile(0.5 * (box.low + box.high), (N, 1))
    t = dict(act_host=act_host, act=torch.as_tensor(act_host, device="cuda:0"), ids=torch.ones(N, dtype=torch.int32, device="cuda:0"),
             field=np.zeros((8, 16)), tq3_host=np.zeros((N, 10)), tq3=torch.zeros((N, 10), dtype=torch.float64, device="cuda:0"),
             bufs=dict(obs=torch.empty((N, 26), dtype=torch.float64, device="cuda:0"), reward=torch.empty(N, dtype=torch.float64, device="cuda:0"),
                       done=torch.empty(N, dtype=torch.uint8, device="cuda:0")))
    for _ in range(2):
        _cycle(traj, t)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        _cycle(traj, t)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    print("free memory: %d bytes after the warm-up, %d after twenty more cycles (bound: %d lower)" % (free0, free1, STATE_ARRAY_BYTES))
    assert free0 - free1 <= STATE_ARRAY_BYTES, (free0, free1)
