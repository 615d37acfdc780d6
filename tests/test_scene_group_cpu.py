"""Scene groups without a GPU: the grouped entry points exist, their blocks have the header's layout and are checked on the host before any
HIP call, and SceneGroup refuses bad arguments before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndet_scene_group_check", "ndet_scene_accumulate_group", "ndet_scene_density_finish_group", "ndet_scene_volume_finish_group")


def test_symbols_and_version():
    from nerfdet_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ndet_version() == 110      # callers probe the grouped entry points by symbol


def _header_struct(name):
    txt = open(os.path.join(ROOT, "include", "nerfdet_hip.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", txt, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)(\s*\*)?\s+(.*)", decl)
        ctype = m.group(2) + ("*" if m.group(3) else "")
        for nm in m.group(4).split(","):
            nm = nm.strip()
            arr = re.match(r"(\w+)\[(\w+)\]", nm)
            fields.append((arr.group(1), ctype, arr.group(2)) if arr else (nm, ctype, None))
    return fields


def test_block_layouts_match_the_header():
    from nerfdet_amd import _lib
    assert ctypes.sizeof(_lib.NdetSceneSlot) == 64
    assert _lib.NDET_GROUP_MAX == 64 and "#define NDET_GROUP_MAX 64" in open(os.path.join(ROOT, "include", "nerfdet_hip.h")).read()
    widths = {"int32_t": 4, "int64_t": 8, "float*": 8, "int32_t*": 8, "NdetSceneSlot*": 8}
    for name in ("NdetSceneSlot", "NdetSceneGroup", "NdetGroupSel"):
        cls = getattr(_lib, name)
        declared = _header_struct(name)
        assert [f[0] for f in cls._fields_] == [d[0] for d in declared], name
        off = 0
        for (fname, ctype, arr) in declared:       # natural alignment, in declaration order: the C compiler's layout
            width = widths[ctype]
            count = 1 if arr is None else (64 if arr == "NDET_GROUP_MAX" else int(arr))
            off = (off + width - 1) // width * width
            field = getattr(cls, fname)
            assert (field.offset, field.size) == (off, width * count), f"{name}.{fname}"
            off += width * count
        assert ctypes.sizeof(cls) == (off + 7) // 8 * 8, name
    assert ctypes.sizeof(_lib.NdetGroupSel) == 8 + 2 * 4 * 64


def _group(**over):
    from nerfdet_amd import _lib
    fields = dict(size=ctypes.sizeof(_lib.NdetSceneGroup), n_slots=3, N=64, C=32, cm=8, k1_pitch=32, k2_pitch=36, table=0x1000)
    fields.update(over)
    return _lib.NdetSceneGroup(**fields)


def _sel(slots=(2, 0), n_views=None, **over):
    from nerfdet_amd import _lib
    sel = _lib.NdetGroupSel(size=ctypes.sizeof(_lib.NdetGroupSel), n=len(slots))
    for i, s in enumerate(slots):
        sel.slot[i] = s
        sel.n_views[i] = 0 if n_views is None else n_views[i]
    for k, v in over.items():
        setattr(sel, k, v)
    return sel


def test_blocks_are_checked_before_any_launch():
    from nerfdet_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)

    def accumulate(g, sel, k=3):
        return lib.ndet_scene_accumulate_group(None if g is None else ctypes.byref(g), None if sel is None else ctypes.byref(sel), k, f, 4, 4, 512, 128,
                                               f, 128, 32, f, f, 16, 16, 768, 256, 16, f, f, None, None)

    def density(g, sel, k=0):
        return lib.ndet_scene_density_finish_group(None if g is None else ctypes.byref(g), None if sel is None else ctypes.byref(sel), f, f, None)

    def volume(g, sel, k=0):
        return lib.ndet_scene_volume_finish_group(None if g is None else ctypes.byref(g), None if sel is None else ctypes.byref(sel), None, f, f, None)

    def check(g, sel, k=3):
        return lib.ndet_scene_group_check(None if g is None else ctypes.byref(g), None if sel is None else ctypes.byref(sel), k)

    assert check(_group(), _sel()) == 0 and check(_group(), _sel(), 0) == 0
    assert check(_group(n_slots=64), _sel(tuple(range(63, -1, -1)))) == 0
    for call in (accumulate, density, volume, check):
        assert call(None, _sel()) == -1 and b"null" in lib.ndet_last_error()
        assert call(_group(), None) == -1 and b"null" in lib.ndet_last_error()
        assert call(_group(size=ctypes.sizeof(_lib.NdetSceneGroup) - 8), _sel()) == -1 and b"size" in lib.ndet_last_error()
        assert call(_group(), _sel(size=ctypes.sizeof(_lib.NdetGroupSel) - 4)) == -1 and b"size" in lib.ndet_last_error()
        assert call(_group(table=0), _sel()) == -1
        assert call(_group(n_slots=0), _sel()) == -1 and call(_group(n_slots=65), _sel()) == -1
        assert call(_group(), _sel(n=0)) == -1 and call(_group(n_slots=64), _sel(n=65)) == -1
        assert call(_group(), _sel((0, 3))) == -1 and b"outside" in lib.ndet_last_error()
        assert call(_group(), _sel((0, -1))) == -1
        assert call(_group(), _sel((1, 2, 1))) == -1 and b"twice" in lib.ndet_last_error()
        assert call(_group(C=30), _sel()) == -2 and call(_group(cm=6), _sel()) == -2
        assert call(_group(k1_pitch=16), _sel()) == -1 and call(_group(k2_pitch=32), _sel()) == -1
        assert call(_group(), _sel(n_views=(0, -1))) == -1
    # view totals that would overflow int32 with the call's k views
    assert accumulate(_group(), _sel(n_views=(5, 0x7fffffff - 2))) == -2 and b"overflows" in lib.ndet_last_error()
    assert check(_group(), _sel(n_views=(5, 0x7fffffff - 3))) == 0
    # k outside 1 .. 128; the accumulate's own inputs
    assert accumulate(_group(), _sel(), 0) == -2 and accumulate(_group(), _sel(), 129) == -2
    assert lib.ndet_scene_accumulate_group(ctypes.byref(_group()), ctypes.byref(_sel()), 3, None, 4, 4, 512, 128, f, 128, 32, f, f, 16, 16, 768, 256, 16,
                                           f, f, None, None) == -1
    assert lib.ndet_scene_accumulate_group(ctypes.byref(_group()), ctypes.byref(_sel()), 3, f, 4, 4, 512, 64, f, 128, 32, f, f, 16, 16, 768, 256, 16,
                                           f, f, None, None) == -1
    assert lib.ndet_scene_volume_finish_group(ctypes.byref(_group()), ctypes.byref(_sel()), None, ctypes.c_void_p(0x1004), f, None) == -2


class _Det:
    training = False
    render_testing = False


def _metas(n, **over):
    from nerfdet_amd.synth import ring_scene_meta
    out = []
    for i in range(n):
        m = ring_scene_meta(6, (64, 96), origin=(0.1 * i, 0.0, 0.5))
        m.update(over)
        out.append(m)
    return out


def _chunk(meta, k, **lidar):
    m = dict(meta)
    m["lidar2img"] = dict(meta["lidar2img"], extrinsic=meta["lidar2img"]["extrinsic"][:k], **lidar)
    return m


def _scene_group(metas):
    from nerfdet_amd.streaming import SceneGroup
    g = SceneGroup.__new__(SceneGroup)        # the checks below run before anything touches a device
    g.det, g.metas = _Det(), metas
    return g


def test_begin_scenes_refuses_bad_groups():
    from nerfdet_amd.detector import nerfdet
    from nerfdet_amd.streaming import SceneGroup
    assert callable(getattr(nerfdet, "begin_scenes"))
    for n in (0, 65):
        with pytest.raises(ValueError, match="1 to 64"):
            SceneGroup(_Det(), _metas(n))
    metas = _metas(3)
    metas[2]["img_shape"] = (60, 96, 3)
    with pytest.raises(ValueError, match="img_shape"):
        SceneGroup(_Det(), metas)
    metas = _metas(2)
    metas[1]["ori_shape"] = (120, 192, 3)
    with pytest.raises(ValueError, match="ori_shape"):
        SceneGroup(_Det(), metas)
    det = _Det()
    det.training = True
    with pytest.raises(RuntimeError, match="inference only"):
        SceneGroup(det, _metas(2))
    det = _Det()
    det.render_testing = True
    with pytest.raises(NotImplementedError):
        SceneGroup(det, _metas(2))


def test_add_views_refuses_bad_calls():
    metas = _metas(3)
    g = _scene_group(metas)
    img = torch.zeros(3, 2, 3, 64, 96)
    chunks = [_chunk(m, 2) for m in metas]
    # duplicate, out-of-range and empty scene lists
    for scenes in ([0, 0], [1, 2, 1], [3], [-1], [], [True]):
        with pytest.raises(ValueError):
            g.add_views(img[:max(len(scenes), 1)], img[:max(len(scenes), 1)], chunks[:len(scenes)], scenes=scenes)
    # k = 0 and 129
    with pytest.raises(ValueError, match="k=0"):
        g.add_views(torch.zeros(3, 0, 3, 64, 96), torch.zeros(3, 0, 3, 64, 96), chunks)
    with pytest.raises(ValueError, match="k=129"):
        g.add_views(torch.zeros(3, 129, 3, 8, 8), torch.zeros(3, 129, 3, 8, 8), chunks)
    # shapes that do not match the listed scenes
    with pytest.raises(ValueError, match="one chunk per listed scene"):
        g.add_views(img[:2], img[:2], chunks)
    with pytest.raises(ValueError, match="one chunk per listed scene"):
        g.add_views(img, img, chunks[:2], scenes=[0, 1])
    with pytest.raises(ValueError, match="denorm_images"):
        g.add_views(img, torch.zeros(3, 1, 3, 64, 96), chunks)
    with pytest.raises(ValueError, match="chunk metas"):
        g.add_views(img, img, chunks[:2])
    with pytest.raises(ValueError, match="depth"):
        g.add_views(img, img, chunks, depth=torch.zeros(3, 3, 8, 8))
    # every row's meta against its own scene
    with pytest.raises(ValueError, match="extrinsics"):
        g.add_views(img, img, [chunks[0], _chunk(metas[1], 3), chunks[2]])
    with pytest.raises(ValueError, match="origin"):
        g.add_views(img, img, [chunks[1], chunks[0], chunks[2]])           # scene 0 handed scene 1's rig
    with pytest.raises(ValueError, match="origin"):
        g.add_views(img[:2], img[:2], [chunks[0], chunks[2]], scenes=[2, 0])   # listed order, not slot order
    intr = np.array(metas[1]["lidar2img"]["intrinsic"], dtype=np.float32)
    intr[0, 0] *= 1.01
    with pytest.raises(ValueError, match="intrinsic"):
        g.add_views(img, img, [chunks[0], _chunk(metas[1], 2, intrinsic=intr), chunks[2]])
    bad = dict(chunks[2], img_shape=(60, 96, 3))
    with pytest.raises(ValueError, match="img_shape"):
        g.add_views(img, img, [chunks[0], chunks[1], bad])
    g.det = _Det()
    g.det.training = True
    with pytest.raises(RuntimeError, match="inference only"):
        g.add_views(img, img, chunks)


def test_listed_scenes_and_grouped_projections():
    from nerfdet_amd import ops
    assert ops.listed_scenes(4, None) == [0, 1, 2, 3] and ops.listed_scenes(4, [2, 0]) == [2, 0] and ops.listed_scenes(4, (np.int64(3),)) == [3]
    metas = _metas(3)
    chunks = [_chunk(metas[2], 2), _chunk(metas[0], 2)]
    chunks[1]["lidar2img"]["intrinsic"] = np.array(metas[0]["lidar2img"]["intrinsic"], dtype=np.float32) * np.float32(1.25)
    both = ops.compute_projection_group(chunks, (4, 1))
    assert both.shape == (2, 4, 3, 4)
    for j, stride in enumerate((4, 1)):
        assert torch.equal(both[j], torch.cat([ops.compute_projection(c, stride) for c in chunks]))
