"""Every cid_gemm_f16 launch variant the models reach has a strict parity case (tests/gemm_census.py).

* ``test_census_reproduces_fixture`` runs everything the product runs (both UNets through their pipelines, ControlNet, both
  VAE halves, the CLIP towers, the ID stack, the face parser; synthetic weights, no CPU oracle) under the recorder and
  compares the set of variant keys with tests/golden/gemm_calls.json.
* ``test_variant_parity`` is generated from that file: for every variant key outside mode 3 the recorded descriptor with the
  smallest M * N * K is planned (the key must still come out), built from fp16-representable random operands, launched into
  a sentinel-filled output with guard rows / columns, and checked against a plain PyTorch CPU reference of the operation at
  the project's default tolerances; guards bit-untouched, second launch bit-identical, statistics / second destination
  consistent.  Mode 3 (the attention epilogue) is covered by test_gpu_kernels.test_id_cross_attention, which
  tests/test_gemm_plan_host.py holds to the census.
"""
import time

import pytest

import gemm_census
import gemm_parity

pytestmark = pytest.mark.gpu

FIXTURE = gemm_census.load()
KEYS = gemm_census.keys_of(gemm_census.all_records(FIXTURE))
TABLE = {k: rp for k, rp in KEYS.items() if rp[0]["mode"] != 3}


def test_census_reproduces_fixture(dev):
    t0 = time.time()
    census = gemm_census.record_census(dev)
    fresh = {}
    for wl, recs in census.items():
        for d, p in recs:
            rec, plan = dict(zip(gemm_census.DESC_FIELDS, d)), dict(zip(gemm_census.PLAN_FIELDS, p))
            assert rec["stats"] == plan["stats"], f"{wl}: ops.gemm attached statistics ({rec['stats']}) against its plan: {rec} {plan}"
            fresh.setdefault(gemm_census.variant_key(rec, plan), wl)
    print(f"[census] {sum(len(v) for v in census.values())} descriptors, {len(fresh)} variant keys, {time.time() - t0:.0f} s")
    assert set(census) == set(FIXTURE), f"workloads differ: {set(census) ^ set(FIXTURE)}"
    new, gone = sorted(set(fresh) - set(KEYS)), sorted(set(KEYS) - set(fresh))
    msg = "".join(f"\n  + {k}   (first seen in {fresh[k]})" for k in new) + "".join(f"\n  - {k}" for k in gone)
    assert not new and not gone, f"the models reach other launch variants than tests/golden/gemm_calls.json lists:{msg}\n" \
                                 f"regenerate it: {gemm_census.REGENERATE}"


# ----------------------------------------------------------------------------- one parity case per key
@pytest.mark.parametrize("key", list(TABLE))
def test_variant_parity(dev, key):
    rec, plan = TABLE[key]
    gemm_parity.run_case(dev, key, rec, plan)
