import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` through gpurun)")


def load_golden(name):
    """npz fixture -> dict of torch tensors (numpy scalars/ints kept as numpy)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {}
    for k in z.files:
        a = z[k]
        out[k] = torch.from_numpy(a) if a.ndim > 0 and a.dtype.kind in "fiub" else a
    return out


def golden_meta(g):
    """rebuild the img_meta dict a golden fixture was generated with."""
    return dict(
        lidar2img=dict(intrinsic=g["intrinsic"].numpy(), extrinsic=[e for e in g["extrinsic"].numpy()],
                       origin=g["origin"].numpy()),
        ori_shape=tuple(int(v) for v in g["ori_shape"]), img_shape=tuple(int(v) for v in g["img_shape"]))


def reference_config_names():
    """File names of the reference's configs/nerfdet/*.py, as stored in golden/nerfdet_configs.json."""
    import json
    with open(os.path.join(GOLDEN, "nerfdet_configs.json")) as f:
        return sorted(json.load(f))


def reference_config(directory, name):
    """Path of a flat config file that ``Config.fromfile`` reads as the reference's configs/nerfdet/<name>: the values stored in
    golden/nerfdet_configs.json (make_golden_configs.py) written out as one ``key = literal`` line each."""
    import json
    with open(os.path.join(GOLDEN, "nerfdet_configs.json")) as f:
        cfg = json.load(f, object_hook=lambda d: tuple(d["__tuple__"]) if set(d) == {"__tuple__"} else d)[name]
    path = os.path.join(str(directory), name)
    with open(path, "w") as f:
        f.writelines(f"{k} = {v!r}\n" for k, v in cfg.items())
    return path


def sub_state(g, prefix):
    return {k[len(prefix):]: torch.as_tensor(v) for k, v in g.items() if k.startswith(prefix)}


@pytest.fixture(scope="session")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")
