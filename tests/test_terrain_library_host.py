"""Terrain library, host side (no GPU): the PNG library loader, the per-environment terrain draw and its independence of the rank split,
input checks, and the terrain spec a TRPO snapshot records."""
import glob
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from cassierl_amd import terrain as T

PNGS = sorted(glob.glob(os.path.join(GOLDEN, "*.png")))


def test_library_from_pngs_equals_hfield_from_png():
    assert PNGS
    size = (10.0, 10.0, 0.2, 0.001)
    lib = T.library_from_pngs(PNGS + PNGS[:1], size)
    assert len(lib) == len(PNGS) + 1
    for f, p in zip(lib, PNGS + PNGS[:1]):
        ref = T.hfield_from_png(p, size)
        assert f.dtype == np.float64 and f.shape == ref.shape
        assert np.array_equal(f, ref)


def test_assign_terrains_does_not_depend_on_the_rank_split():
    n, k = 1000, 7
    one = T.assign_terrains(3, torch.arange(n), k)
    assert one.dtype == torch.int32 and one.shape == (n,)
    assert int(one.min()) >= 0 and int(one.max()) < k
    assert len(torch.unique(one)) == k                        # every field is drawn at this size
    two = torch.cat([T.assign_terrains(3, torch.arange(0, 600), k), T.assign_terrains(3, torch.arange(600, n), k)])
    assert torch.equal(one, two)
    assert not torch.equal(one, T.assign_terrains(4, torch.arange(n), k))   # the seed matters
    assert torch.equal(T.assign_terrains(3, torch.arange(n), 1), torch.zeros(n, dtype=torch.int32))


def test_bad_inputs_raise():
    with pytest.raises(ValueError):
        T.assign_terrains(1, torch.arange(4), 0)
    with pytest.raises(ValueError):
        T.assign_terrains(1, torch.zeros((2, 2), dtype=torch.int64), 3)
    with pytest.raises(ValueError):
        T.library_from_pngs([], (10, 10, 1, 0.001))
    with pytest.raises(ValueError):
        T.library_from_pngs(PNGS, (0.0, 10.0, 1.0, 0.001))
    with pytest.raises(ValueError):
        T.library_from_pngs(PNGS, (10.0, 10.0))
    with pytest.raises(ValueError):
        T.terrain_spec(os.path.dirname(PNGS[0]), 1, -1.0, 1)


def test_vec_env_library_checks_its_fields_before_any_call():
    """set_terrain_library refuses field shapes and sizes before it reaches the library (no handle is needed to get there)."""
    from cassierl_amd.vec_env import CassieVecEnv
    env = CassieVecEnv.__new__(CassieVecEnv)   # no device: the checks come first
    good = np.zeros((4, 5))
    with pytest.raises(ValueError):
        env.set_terrain_library([good, np.zeros(5)])
    with pytest.raises(ValueError):
        env.set_terrain_library([good, np.zeros((1, 5))])
    with pytest.raises(ValueError):
        env.set_terrain_library([good, good], sizes=[(10, 10)] * 3)


def test_terrain_spec_draw_is_seeded_and_keyed(tmp_path):
    for i in range(6):
        shutil.copy(PNGS[0], os.path.join(str(tmp_path), "t%d.png" % i))
    a = T.terrain_spec(str(tmp_path), 5, 0.05, 11)
    b = T.terrain_spec(str(tmp_path), 5, 0.05, 11)
    assert a == b and len(a["files"]) == 5 and set(a["files"]) <= {"t%d.png" % i for i in range(6)}
    key = T.spec_key(a)
    assert key == dict(files=a["files"], elevation=0.05, seed=11, num_terrains=5) and T.spec_key(None) is None
    assert T.spec_key(dict(a, dir="/elsewhere")) == key                       # where the files live is not part of the ground
    assert T.spec_key(dict(a, elevation=0.06)) != key
    lib = T.library_of_spec(a)
    assert len(lib) == 5
    for f in lib:   # lowered so that the reset pose stands clear: the highest point under the feet is just below the floor
        top = max(T.height_at(f, 10, 10, x, y) for x in np.linspace(-0.2, 0.3, 26) for y in (-0.1305, 0.1305))
        assert -2e-4 < top < 0.0
