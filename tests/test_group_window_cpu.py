"""Windowed scene groups without a GPU: the grouped ring finishes exist, their selection block has the header's layout, the pool block, the
selection and the segment lists are checked on the host before any HIP call, and a windowed SceneGroup keeps its windows' books --
independent eviction, refusals that change nothing -- with the grouped accumulate replaced by a recorder."""
import ctypes
import inspect
import os

import pytest
import torch

from test_scene_group_cpu import ROOT, _Det, _header_struct, _metas, _scene_group

NAMES = ("ndet_scene_group_ring_check", "ndet_scene_density_finish_group_ring", "ndet_scene_volume_finish_group_ring")
POOL_MAX = 64 * 65


def test_symbols_and_version():
    from nerfdet_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ndet_version() == 110      # callers probe the new entry points by symbol


def test_selection_layout_matches_the_header():
    from nerfdet_amd import _lib, ops
    cls = _lib.NdetGroupRingSel
    declared = _header_struct("NdetGroupRingSel")
    assert [f[0] for f in cls._fields_] == [d[0] for d in declared] == ["size", "n", "n_segs", "n_views"]
    off = 0
    for fname, ctype, arr in declared:
        assert ctype == "int32_t" and arr in (None, "NDET_GROUP_MAX")
        count = 1 if arr is None else 64
        field = getattr(cls, fname)
        assert (field.offset, field.size) == (off, 4 * count), fname
        off += 4 * count
    assert ctypes.sizeof(cls) == off == 520
    header = open(os.path.join(ROOT, "include", "nerfdet_hip.h")).read()
    assert "#define NDET_GROUP_POOL_MAX (NDET_GROUP_MAX * (NDET_RING_MAX + 1))" in header
    assert "#define NDET_GROUP_MAX 64" in header and "#define NDET_RING_MAX 64" in header
    assert _lib.NDET_GROUP_POOL_MAX == POOL_MAX and ops.GROUP_POOL_MAX == POOL_MAX


def _pool(**over):
    from nerfdet_amd import _lib
    fields = dict(size=ctypes.sizeof(_lib.NdetSceneGroup), n_slots=9, N=64, C=32, cm=8, k1_pitch=32, k2_pitch=36, table=0x1000)
    fields.update(over)
    return _lib.NdetSceneGroup(**fields)


def _sel(lists=((4, 0, 7), (2,)), n_views=None, n_segs=None, **over):
    """``(NdetGroupRingSel, (n, 64) int32 segment lists)`` for the per-scene lists of pool rows."""
    from nerfdet_amd import _lib
    sel = _lib.NdetGroupRingSel(size=ctypes.sizeof(_lib.NdetGroupRingSel), n=len(lists))
    segs = torch.full((max(len(lists), 1), 64), -7, dtype=torch.int32)        # entries beyond n_segs[i] are never read
    for i, rows in enumerate(lists):
        sel.n_segs[i] = len(rows) if n_segs is None else n_segs[i]
        sel.n_views[i] = 3 * len(rows) if n_views is None else n_views[i]
        segs[i, :len(rows)] = torch.tensor(rows, dtype=torch.int32)
    for k, v in over.items():
        setattr(sel, k, v)
    return sel, segs


def test_blocks_and_lists_are_checked_before_any_launch():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)

    def args(g, sel_segs, host=True):
        sel, segs = sel_segs
        return (None if g is None else ctypes.byref(g), None if sel is None else ctypes.byref(sel),
                ctypes.c_void_p(segs.data_ptr()) if host else None)

    def check(g, sel_segs, host=True, dev=f):
        return lib.ndet_scene_group_ring_check(*args(g, sel_segs, host))

    def density(g, sel_segs, host=True, dev=f):
        return lib.ndet_scene_density_finish_group_ring(*args(g, sel_segs, host), dev, f, f, None)

    def volume(g, sel_segs, host=True, dev=f):
        return lib.ndet_scene_volume_finish_group_ring(*args(g, sel_segs, host), dev, None, f, f, None)

    def err():
        return lib.ndet_last_error()

    # accepted calls go through the check alone: the finishes would launch them
    assert check(_pool(), _sel()) == 0
    assert check(_pool(), _sel(n_views=(0, 0))) == 0
    full = tuple(tuple(range(65 * i, 65 * i + 64)) for i in range(64))       # 64 scenes of 64 segments in the largest table
    assert check(_pool(n_slots=POOL_MAX), _sel(full)) == 0
    assert check(_pool(n_slots=POOL_MAX), _sel(((POOL_MAX - 1, 0),))) == 0
    for call in (check, density, volume):
        assert call(None, _sel()) == -1 and b"null" in err()
        assert call(_pool(), (None, _sel()[1])) == -1 and b"null" in err()
        assert call(_pool(size=ctypes.sizeof(_lib.NdetSceneGroup) - 8), _sel()) == -1 and b"size" in err()
        assert call(_pool(), _sel(size=ctypes.sizeof(_lib.NdetGroupRingSel) - 4)) == -1 and b"size" in err()
        assert call(_pool(), _sel(size=ctypes.sizeof(_lib.NdetGroupSel) + 4)) == -1 and b"size" in err()
        assert call(_pool(), _sel(n=0)) == -1 and call(_pool(n_slots=POOL_MAX), _sel(full, n=65)) == -1 and b"listed scenes" in err()
        assert call(_pool(), _sel(n_segs=(0, 1))) == -1 and b"n_segs[0]=0" in err()
        assert call(_pool(), _sel(n_segs=(3, 65))) == -1 and b"n_segs[1]=65" in err()
        assert call(_pool(), _sel(((4, -1, 7), (2,)))) == -1 and b"outside" in err()
        assert call(_pool(), _sel(((4, 0, 7), (9,)))) == -1 and b"segs[1][0]=9" in err() and b"outside" in err()
        assert call(_pool(), _sel(((4, 0, 4), (2,)))) == -1 and b"twice" in err()          # within a scene
        assert call(_pool(), _sel(((4, 0, 7), (2, 0)))) == -1 and b"segs[1][1]=0" in err() and b"twice" in err()     # across scenes
        assert call(_pool(), _sel(n_views=(3, -1))) == -1 and b"n_views[1]" in err()
        assert call(_pool(n_slots=0), _sel()) == -1 and call(_pool(n_slots=POOL_MAX + 1), _sel()) == -1 and b"n_slots" in err()
        assert call(_pool(table=0), _sel()) == -1
        assert call(_pool(C=30), _sel()) == -2 and call(_pool(cm=6), _sel()) == -2
        assert call(_pool(k1_pitch=16), _sel()) == -1 and call(_pool(k2_pitch=32), _sel()) == -1
        assert call(_pool(), _sel(), host=False) == -1 and b"null segs_host" in err()
    for call in (density, volume):
        assert call(_pool(), _sel(), dev=None) == -1 and b"null segs_dev" in err()
    # the outputs' alignments, as the single-scene ring finishes require them
    g, (sel, segs) = _pool(), _sel()
    a = args(g, (sel, segs))
    assert lib.ndet_scene_density_finish_group_ring(*a, f, None, f, None) == -1 and b"null bias" in err()
    assert lib.ndet_scene_density_finish_group_ring(*a, f, f, None, None) == -1 and b"null global_feat" in err()
    assert lib.ndet_scene_density_finish_group_ring(*a, f, f, ctypes.c_void_p(0x1004), None) == -2 and b"global_feat" in err()
    assert lib.ndet_scene_volume_finish_group_ring(*a, f, None, None, f, None) == -1 and b"null out" in err()
    assert lib.ndet_scene_volume_finish_group_ring(*a, f, None, f, None, None) == -1 and b"null count" in err()
    assert lib.ndet_scene_volume_finish_group_ring(*a, f, None, ctypes.c_void_p(0x1008), f, None) == -2 and b"out must be 16-byte aligned" in err()
    assert lib.ndet_scene_volume_finish_group_ring(*a, f, None, f, ctypes.c_void_p(0x1004), None) == -2 and b"count must be 8-byte aligned" in err()


def test_unwindowed_entry_points_keep_their_bound():
    from nerfdet_amd import _lib
    lib = _lib.load()
    sel = _lib.NdetGroupSel(size=ctypes.sizeof(_lib.NdetGroupSel), n=1)
    assert lib.ndet_scene_group_check(ctypes.byref(_pool(n_slots=64)), ctypes.byref(sel), 0) == 0
    assert lib.ndet_scene_group_check(ctypes.byref(_pool(n_slots=65)), ctypes.byref(sel), 0) == -1 and b"n_slots=65" in lib.ndet_last_error()


# ---- SceneGroup(window=) ----
GRID, C, CM = (2, 2, 2), 8, 4


def _windowed(n, window):
    """A windowed SceneGroup on the CPU, built as test_scene_group_cpu._scene_group builds an unwindowed one."""
    from nerfdet_amd import ops
    g = _scene_group(_metas(n))
    g.window = window
    g.pool = ops.SceneGroupRingState(GRID, C, CM, [torch.zeros(3, *GRID) for _ in range(n)], window, "cpu")
    return g


def test_window_and_drop_oldest_are_validated():
    from nerfdet_amd import ops
    from nerfdet_amd.detector import nerfdet
    from nerfdet_amd.streaming import SceneGroup
    assert inspect.signature(nerfdet.begin_scenes).parameters["window"].default is None
    for w in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="window"):
            SceneGroup(_Det(), _metas(2), window=w)
        with pytest.raises(ValueError, match="window"):
            ops.SceneGroupRingState(GRID, C, CM, [torch.zeros(3, *GRID)], w, "cpu")
    plain = _scene_group(_metas(2))
    assert plain.window is None
    with pytest.raises(ValueError, match="windowed"):
        plain.drop_oldest()
    g = _windowed(3, 2)
    with pytest.raises(ValueError, match="k=1"):
        g.drop_oldest(1)
    g.drop_oldest(0)
    for st, s in zip(g.pool.take([0, 1]), (0, 1)):
        st.n_views = 4
        g.pool.push([s], [st])
    assert g.n_chunks == [1, 1, 0]
    with pytest.raises(ValueError, match="k=1"):
        g.drop_oldest(1)                      # scene 2 holds nothing: the call is refused whole
    with pytest.raises(ValueError, match="k=2"):
        g.drop_oldest(2, scenes=[0, 1])
    for k in (-1, True, 1.0):
        with pytest.raises(ValueError):
            g.drop_oldest(k, scenes=[0])
    with pytest.raises(ValueError):
        g.drop_oldest(1, scenes=[0, 0])
    assert g.n_chunks == [1, 1, 0] and g.n_views == [4, 4, 0]
    g.drop_oldest(1, scenes=[1])
    assert g.chunk_views == [[4], [], []]
    with pytest.raises(ValueError, match="no views"):
        g.volume()
    g.reset()
    assert g.n_views == [0, 0, 0] and [len(s) for s in g.pool.spare] == [1, 1, 0]


def _recorder(monkeypatch):
    from nerfdet_amd import ops
    calls = []

    def fill(pool, scenes, *chunk, depth_gate=None, states=None):
        calls.append((list(scenes), chunk[0]))
        assert states is not None and len(states) == len(scenes) and all(st.n_views == 0 and not st.k1_sum.any() for st in states)
        if chunk[0] == "bad":
            for st in states:
                st.k1_sum.fill_(1.0)
            raise RuntimeError("boom")
        for st in states:
            st.n_views = chunk[0]

    monkeypatch.setattr(ops, "scene_accumulate_group_ring", fill)
    return calls


def test_scenes_evict_independently(monkeypatch):
    calls = _recorder(monkeypatch)
    g = _windowed(3, 2)
    g._accumulate([0, 1, 2], 3)
    g._accumulate([2, 0], 5)
    assert g.chunk_views == [[3, 5], [3], [3, 5]] and g.n_chunks == [2, 1, 2] and g.n_views == [8, 3, 8]
    oldest = [segs[0] for segs in g.pool.segs]
    g._accumulate([0], 7)                      # scene 0's window was full: its oldest chunk leaves, the others keep theirs
    assert g.chunk_views == [[5, 7], [3], [3, 5]]
    assert g.pool.spare[0] == [oldest[0]] and oldest[0].n_views == 0 and g.pool.segs[1][0] is oldest[1] and g.pool.segs[2][0] is oldest[2]
    g._accumulate([1, 2], 2)
    assert g.chunk_views == [[5, 7], [3, 2], [5, 2]] and g.n_views == [12, 5, 7]
    g._accumulate([0, 1, 2], 1)                # steady state for scene 0: the state that left is the one filled, nothing is allocated
    assert g.chunk_views == [[7, 1], [2, 1], [2, 1]] and g.pool.segs[0][1] is oldest[0]
    g.drop_oldest(1, scenes=[2])
    g.reset(scenes=[1])
    assert g.chunk_views == [[7, 1], [], [1]] and g.n_chunks == [2, 0, 1] and g.n_views == [8, 0, 1]
    assert calls == [([0, 1, 2], 3), ([2, 0], 5), ([0], 7), ([1, 2], 2), ([0, 1, 2], 1)]
    # every state is a pool row of its scene's
    for s in range(3):
        for st in g.pool.segs[s] + g.pool.spare[s]:
            assert g.pool.states[st.row] is st and g.pool.owner[st.row] == s


def test_a_failing_accumulate_leaves_every_window_as_it_was(monkeypatch):
    _recorder(monkeypatch)
    g = _windowed(3, 2)
    g._accumulate([0, 1, 2], 3)
    g._accumulate([0, 1], 5)
    segs = [list(s) for s in g.pool.segs]
    spare = [list(s) for s in g.pool.spare]
    with pytest.raises(RuntimeError, match="boom"):
        g._accumulate([2, 0], "bad")
    assert g.chunk_views == [[3, 5], [3, 5], [3]]
    assert all(a == b and all(x is y for x, y in zip(a, b)) for a, b in zip(g.pool.segs, segs))
    # the states the call took went back, zeroed: scene 0's was newly allocated (its window was full), scene 2's too; scene 1 owns none
    assert [len(s) for s in g.pool.spare] == [len(spare[0]) + 1, len(spare[1]), len(spare[2]) + 1]
    for s in (0, 2):
        assert not g.pool.spare[s][-1].k1_sum.any() and g.pool.spare[s][-1].n_views == 0
    g._accumulate([2, 0], 7)                    # the same states serve the call that follows
    assert g.chunk_views == [[5, 7], [3, 5], [3, 7]] and [g.pool.owned(s) for s in range(3)] == [3, 2, 2]


def test_a_sliding_window_owns_at_most_window_plus_one_states(monkeypatch):
    _recorder(monkeypatch)
    for window in (1, 3):
        g = _windowed(2, window)
        for r in range(3 * window + 2):
            g._accumulate([0, 1] if r % 3 else [1], r + 1)
            if r == window + 1:
                with pytest.raises(RuntimeError):
                    g._accumulate([0, 1], "bad")
            assert all(g.pool.owned(s) <= window + 1 for s in range(2)), (window, r)
            assert all(n <= window for n in g.n_chunks)
        assert g.pool.owned(1) == window + 1 and len(g.pool.states) <= 2 * (window + 1)
        assert g.n_chunks[1] == window
