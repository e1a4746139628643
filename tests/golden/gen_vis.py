"""Generate tests/golden/vis_loop600_icp.npz: the 599 stage-1 edges of
``make_loop_sequence(600, 3)`` as oracle/icp_oracle.py computes them from the
odometry inits (epsilon 0.05, 100 iterations at most), which the device ICP
matches.  About three minutes on one CPU core, which is why tests/test_vis.py
reads the file instead of computing the edges (it recomputes a few of them and
compares).  The .npz holds the transforms only (data, no code).

    python tests/golden/gen_vis.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "icp-slam-with-loop-closure_amd"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import icp_oracle  # noqa: E402
from slamhip import se2, synthetic  # noqa: E402


def oracle_edge(seq, i):
    """The oracle's icp(pc1 = scan i, pc2 = scan i - 1) from the odometry init."""
    init = se2.pose_to_mat(seq.odometry[i] - seq.odometry[i - 1])
    hist, _ = icp_oracle.icp(synthetic.homogeneous(seq.scans[i]), synthetic.homogeneous(seq.scans[i - 1]),
                             init.copy(), 0.05, 100)
    return np.array(hist[-1])


def main():
    seq = synthetic.make_loop_sequence(600, 3)
    tf = np.stack([oracle_edge(seq, i) for i in range(1, len(seq.scans))])
    np.savez_compressed(os.path.join(HERE, "vis_loop600_icp.npz"), tf=tf)
    print("wrote", tf.shape)


if __name__ == "__main__":
    main()
