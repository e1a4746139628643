"""Writes tests/golden/loc_e2e_map.npz: the occupancy grid of the localisation
experiment (tests/loc_ref.py: e2e_inputs) built by oracle/occupancy_oracle.py on
the CPU, so that tests/test_loc.py needs neither a GPU nor the oracle's six
seconds.  tests/test_loc_gpu.py checks that produce_occupancy_grid gives the
same grid.

    python tests/golden/gen_loc.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "icp-slam-with-loop-closure_amd"), os.path.join(REPO, "oracle"),
                os.path.join(REPO, "tests")]

import loc_ref  # noqa: E402
import occupancy_oracle  # noqa: E402

if __name__ == "__main__":
    seq, map_idx, _, _ = loc_ref.e2e_inputs()
    grid, origin = occupancy_oracle.produce(seq.truth[map_idx], [seq.scans[i] for i in map_idx],
                                            loc_ref.E2E["cell_width"])
    np.savez_compressed(os.path.join(HERE, "loc_e2e_map.npz"), grid=grid, origin=np.asarray(origin, dtype=np.float64),
                        cell_width=np.float64(loc_ref.E2E["cell_width"]))
    print(grid.shape, origin, int((grid > 0).sum()), "occupied")
