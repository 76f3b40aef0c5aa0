#!/usr/bin/env python
"""One shape per launch-path combination of the transformer block (tests/transformer_paths.py): every level of the SD1.5 UNet,
the SDXL UNet and the SD1.5 ControlNet encoder on the grid of CFG batches and latent sizes there is put through
``transformer_paths.predict`` (host predicates of ops.py / unet.py under the default switches), and the smallest shape of each
combination goes to tests/golden/transformer_paths.json (integers and names only).  A combination whose every shape exceeds
``transformer_paths.MAX_TOKENS`` is listed under "omitted" with that reason.  Under "long": the same walk at 154 + 4, 231 + 4 and
158 + 0 context rows, filed under the fields a long context changes, and one 1280-channel shape per family at 1024 text rows.

Run (no GPU needed):  python tests/golden/make_golden_transformer_paths.py [output path]  ->  tests/golden/transformer_paths.json
"""
import os
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
sys.path.insert(0, str(OUT.parent.parent))

import transformer_paths as tp  # noqa: E402


def main():
    from consistentid_amd import build
    build.build(verbose=False)
    changed = {k: os.environ[k] for k, v in tp.SWITCHES.items() if os.environ.get(k, v) != v}
    assert not changed, f"the table is for the default switches, unset {changed}"
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else tp.GOLDEN
    cases, omitted = {}, {}
    for family in tp.FAMILIES:
        found = tp.enumerate_grid(family)
        cases[family] = {k: shp for k, shp in found.items() if shp is not None}
        omitted[family] = [(k, f"every shape of the grid has more than {tp.MAX_TOKENS} tokens")
                           for k, shp in found.items() if shp is None]
        before = tp.combinations_of(family, tp.COVERED_BEFORE[family])
        print(f"{family}: {len(found)} combinations, {len(cases[family])} with a case, {len(omitted[family])} omitted, "
              f"{len(before)} reached before, largest case {max(s[5] * tp.padded_tokens(s[0], s[1], s[3], s[4], s[7], s[8]) for s in cases[family].values())} tokens")
    # contexts past 96 rows: one shape per (c, heads, pad, dedup, xattn, tail) of SD1.5 and SDXL, one per width of the
    # ControlNet, and one at the most rows a pipeline takes (transformer_paths.enumerate_long / cap_shape)
    long = {}
    for family in tp.FAMILIES:
        found = tp.enumerate_long(family)
        long[family] = list(found.values()) + [tp.cap_shape(family)]
        print(f"{family}: {len(found)} long-context rows at {tp.LONG_CONTEXT[family]}, one at {tp.CAP_CONTEXT[family]}: "
              f"{long[family][-1]}")
    tp.dump(cases, omitted, long, out)
    print(f"-> {out}")


if __name__ == "__main__":
    main()
