#!/usr/bin/env python3
"""Record the fixtures of tests/test_gpu_phase_share.py (tests/golden/phase_share/*.npz) with
the library of the checked-out commit, on a GPU: the fused env step of Humanoid and Ant on every
step kernel (paired, one env per wave by choice / by an odd env count, runtime tables), TGS and
PGS. The cases, the seeded actions and the rollout are the test's own (imported from it); see its
docstring for what a fixture holds and which commit recorded the committed ones.

Every case is run for MAX_STEPS steps; per task the smallest step count is kept at which every
fixture of the task shows a reset at least two steps back and a non-zero force-sensor observation
in the last step.

    python tools/make_golden_phase_share.py [out_dir]     # default: tests/golden/phase_share"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_gpu_phase_share as T  # noqa: E402

MAX_STEPS = 32


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    for task in T.TASKS:
        runs = {}
        for variant in T.VARIANTS:
            for solver in T.SOLVERS:
                runs[(variant, solver)] = T.rollout(task, variant, solver, MAX_STEPS)

        def ok(steps):
            return all(r["reset"][:steps - 2].any() and np.any(T.sensor_block(r["obs"][steps - 1], na) != 0.0)
                       for r, na in runs.values())

        steps = next((k for k in range(3, MAX_STEPS + 1) if ok(k)), None)
        assert steps is not None, f"{task}: no step count up to {MAX_STEPS} shows a reset and a sensor force"
        for (variant, solver), (r, na) in runs.items():
            path = os.path.join(out_dir, os.path.basename(T.fixture_path(task, variant, solver)))
            np.savez_compressed(path, steps=np.int32(steps), num_actions=np.int32(na),
                                obs=r["obs"][steps - 1], rew=r["rew"][steps - 1], reset=r["reset"][steps - 1],
                                rew_steps=r["rew"][:steps], reset_steps=r["reset"][:steps])
            print(task, variant, solver, "steps", steps, "resets", int(r["reset"][:steps].sum()),
                  "sensor max", float(np.abs(T.sensor_block(r["obs"][steps - 1], na)).max()),
                  os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
