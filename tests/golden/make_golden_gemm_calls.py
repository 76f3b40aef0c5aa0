#!/usr/bin/env python
"""The census of cid_gemm_f16 launches the models make (tests/gemm_census.py): every workload of record_census() is run on
the GPU with synthetic weights while a recorder wraps consistentid_amd.ops.gemm; the deduplicated, pointer-free descriptors
and their plans (integers only) go to tests/golden/gemm_calls.json.

Run (needs the MI355X):  python tests/golden/make_golden_gemm_calls.py [output path]  ->  tests/golden/gemm_calls.json
"""
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
sys.path.insert(0, str(OUT.parent.parent))
import torch  # noqa: E402

import gemm_census  # noqa: E402


def main():
    assert torch.cuda.is_available(), "the census is recorded on the GPU"
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else gemm_census.GOLDEN
    census = gemm_census.record_census(torch.device("cuda:0"))
    out.parent.mkdir(parents=True, exist_ok=True)
    gemm_census.dump(census, out)
    fixture = gemm_census.load(out)
    keys = gemm_census.keys_of(gemm_census.all_records(fixture))
    print(f"{sum(len(v) for v in fixture.values())} descriptors in {len(fixture)} workloads, {len(keys)} variant keys -> {out}")
    for k in keys:
        print("  ", k)


if __name__ == "__main__":
    main()
