#!/usr/bin/env python
"""The characterisation grid of the GEMM planner (tests/gemm_plan_grid.py): the census descriptors of
tests/golden/gemm_calls.json and synthetic neighbours of them are planned by cid_gemm_plan under the default planner switches
and under each non-default value of each switch, every setting in a child process of its own (the switches are read once per
process); return codes, plan fields and refusal texts go to tests/golden/gemm_plan_grid.json.

Run (no GPU needed):  python tests/golden/make_golden_gemm_plan_grid.py [output path]  ->  tests/golden/gemm_plan_grid.json
"""
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
sys.path.insert(0, str(OUT.parent.parent))

import gemm_plan_grid as grid  # noqa: E402


def main():
    from consistentid_amd import build
    build.build(verbose=False)
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else grid.GOLDEN
    descs, neighbours = grid.build_cases()
    grid.dump(descs, neighbours, [], {}, out)              # the children read the cases from the file itself
    default = grid.run_child("plan", out)
    settings = {}
    for s in grid.SETTINGS:
        settings[s] = grid.run_child("plan", out, s)
        print(f"{s}: {sum(r != r0 for r, r0 in zip(settings[s], default))} of {len(default)} cases answer differently")
    grid.dump(descs, neighbours, default, settings, out)
    refused = sum(1 for r in default if r[0])
    print(f"{len(descs)} descriptors + {len(neighbours)} neighbours, {refused} refused under the defaults, "
          f"{1 + len(grid.SETTINGS)} settings -> {out}")


if __name__ == "__main__":
    main()
