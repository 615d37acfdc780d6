#!/usr/bin/env python3
"""Golden vectors of hierarchical sampling from the REAL reference code: ``sample_pdf(det=True)`` of
mmdet3d/models/model_utils/render_ray.py:96-142 on the CPU, at the (S, n_imp) shapes of tests/importance_ref.py with one ray per
weight pattern.  Run in the build container only, like make_golden.py:
    python tests/golden/make_golden_sample_pdf.py
Only inputs (bins, weights) and outputs (samples) are stored: tests/golden/sample_pdf_det.npz.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import make_golden as G  # noqa: E402
import importance_ref as I  # noqa: E402


def main():
    ref = G.load_reference()
    out = {}
    for ci, (s, n) in enumerate(I.SHAPES):
        m = s - 2
        rows_b, rows_w = [], []
        for pi, pattern in enumerate(I.WEIGHT_PATTERNS):
            z = I.coarse_depths(1, s, seed=100 * ci + pi)
            rows_b.append(I.mid_bins(z))
            rows_w.append(I.weights_of(pattern, 1, m, seed=1000 + 100 * ci + pi))
        bins, weights = torch.cat(rows_b).contiguous(), torch.cat(rows_w).contiguous()
        samples = ref.render_ray.sample_pdf(bins.clone(), weights.clone(), n, det=True)     # the reference adds 1e-5 IN PLACE: hand it a clone
        out.update({f"c{ci}_bins": bins.numpy(), f"c{ci}_weights": weights.numpy(), f"c{ci}_samples": samples.numpy(),
                    f"c{ci}_shape": np.asarray([s, n], dtype=np.int64)})
        print(f"(S={s}, n_imp={n}): bins {tuple(bins.shape)}, weights {tuple(weights.shape)}, samples {tuple(samples.shape)}")
    out["patterns"] = np.asarray(I.WEIGHT_PATTERNS)
    path = os.path.join(HERE, "sample_pdf_det.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
