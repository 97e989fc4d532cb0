"""Generates tests/golden/ref_outputs.npz: what the REAL reference libraries (oracle/_ref/*.so, compiled from the reference tree by
oracle/Makefile) return on the seeded inputs of the tests that compare the oracle with them, so that those tests run where oracle/_ref
cannot be built (oracle_lib.reference_outputs; where it can, the tests recompute every entry and require the recording).
Run where the reference tree exists, after `make -C oracle ref`:  python tests/golden/make_ref_outputs.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib  # noqa: E402
import test_ba  # noqa: E402
import test_hkmeans_oracle  # noqa: E402
import test_knn  # noqa: E402
import test_pnp  # noqa: E402
import test_projmatch_oracle  # noqa: E402

groups = {"g2o_ba": ("g2o", test_ba.g2o_ba_outputs), "g2o_ba_hard": ("g2o", test_ba.g2o_ba_hard_outputs),
          "g2o_pnp": ("g2o", test_pnp.g2o_pnp_outputs), "xflann_linear": ("xflann", test_knn.xflann_linear_outputs)}
groups.update({f"xflann_hkmeans_{n}": ("xflann", test_hkmeans_oracle.xflann_hkmeans_outputs(n)) for n in test_hkmeans_oracle._sets()})
groups.update({f"picoflann_radius_{n}": ("picoflann", test_projmatch_oracle.picoflann_radius_outputs(n))
               for n, xy in test_projmatch_oracle._clouds().items() if len(xy)})   # (the empty cloud is not searched)
out = {}
for group, (name, compute) in groups.items():
    ref = oracle_lib.load_ref(name)
    assert ref is not None, f"oracle/_ref/lib{name}_ref.so is missing: build oracle/_ref first (make -C oracle ref)"
    out[f"{group}__index"], out[f"{group}__data"] = oracle_lib.pack_arrays(compute(ref))
np.savez_compressed(os.path.join(HERE, "ref_outputs.npz"), **out)
print("wrote ref_outputs.npz:", len(out) // 2, "groups,", sum(v.nbytes for v in out.values()), "bytes raw")
