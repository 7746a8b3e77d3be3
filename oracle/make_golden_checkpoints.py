#!/usr/bin/env python
"""TEST INFRASTRUCTURE.  A data fixture of the TD3 actor checkpoints the reference ships
(turtlebot3_rl_sim/src/models/td3/**/td3_actor_model_ep*.pt, ~640 KB each): for every checkpoint its path under
models/td3, the state_dict's keys in order, their shapes and dtypes, and the small tensors (every bias, linear3.weight)
verbatim.  tests/test_td3_parity.py rebuilds each state_dict from it and loads it into crowdnav.td3.Actor with strict key
matching, without the reference tree.

Writes tests/golden/td3_checkpoints.npz (data only).  Usage: python oracle/make_golden_checkpoints.py REFERENCE_ROOT"""
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = 4096          # tensors of at most this many elements are stored verbatim


def main(ref_root):
    base = os.path.join(ref_root, "turtlebot3_rl_sim", "src", "models", "td3")
    files = sorted(glob.glob(os.path.join(base, "**", "td3_actor_model_ep*.pt"), recursive=True))
    if not files:
        raise SystemExit("no td3_actor_model_ep*.pt under %s" % base)
    out = {"names": np.array([os.path.relpath(f, base) for f in files])}
    for i, f in enumerate(files):
        sd = torch.load(f, map_location="cpu")
        keys = list(sd.keys())
        out["c%d_keys" % i] = np.array(keys)
        out["c%d_shapes" % i] = np.array([list(sd[k].shape) + [-1] * (2 - sd[k].dim()) for k in keys], dtype=np.int64)
        out["c%d_dtypes" % i] = np.array([str(sd[k].dtype).replace("torch.", "") for k in keys])
        for k in keys:
            if sd[k].numel() <= SMALL:
                out["c%d_t_%s" % (i, k)] = sd[k].numpy()
    path = os.path.join(ROOT, "tests", "golden", "td3_checkpoints.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d checkpoints" % (path, len(files)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
