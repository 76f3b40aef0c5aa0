"""Characterisation grid of the GEMM planner (test helper, not a conftest).

tests/golden/gemm_plan_grid.json pins what ``cid_gemm_plan`` answers -- return code, every ``cid_gemm_plan_info`` field and, on
refusal, the ``cid_last_error()`` text -- for the census descriptors (tests/golden/gemm_calls.json) and synthetic neighbours of
them, under the default planner switches and under each non-default value of each switch, one switch at a time.  The switches
are read once per process, so every setting is planned in a child process of its own (``python tests/gemm_plan_grid.py``).

The file holds integers and short strings only: ``descs`` are full descriptors (FIELDS order; pointers as addresses: 0 = NULL,
64 = present, 72 = present and misaligned), ``neighbours`` are ``[index into descs, {field: value}]`` overrides; the cases are
``descs`` followed by the expanded neighbours.  ``results`` lists every distinct answer once (``[0, *INFO_FIELDS]`` or
``[rc, text]``); ``default`` has one index into it per case, ``settings`` maps "NAME=VALUE" to the cases that answer differently
there (``[case index, result index]`` pairs).
tests/golden/make_golden_gemm_plan_grid.py writes it; tests/test_gemm_plan_host.py replays it without a GPU."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import gemm_census

GOLDEN = Path(__file__).resolve().parent / "golden" / "gemm_plan_grid.json"
REGENERATE = "python tests/golden/make_golden_gemm_plan_grid.py   (no GPU needed; writes tests/golden/gemm_plan_grid.json)"

PTRS = ("x1", "x2", "w", "out", "bias", "rowbias", "res", "vt", "ws", "ln_s", "ln_b", "gn_stats", "att_kp", "att_vp", "att_kvrow",
        "out2", "w_up4")
FIELDS = gemm_census.DESC_INTS + ("ws_bytes", "ln_eps_pos") + PTRS       # ln_eps_pos: ln_eps = 1e-5 (1) or 0 (0)
INFO_FIELDS = ("family", "bm", "bn", "splitk", "nloop", "nbuf", "ln", "act", "vmode", "splitk_epilogue", "stats_rows")

# every planner switch (csrc/gemm_plan.hip, PlanSwitches) with its non-default values; CID_GEMM_ABLATE exists in ablation
# builds only and selects no launch
SETTINGS = ("CID_GEGLU_TILE=1", "CID_GEGLU_TILE=2", "CID_GEMM_TILE=1", "CID_GEMM_TILE=2", "CID_GEMM_TILE=3", "CID_GEMM_SK=2",
            "CID_GEMM_SK=4", "CID_GEMM_PREFER128=0", "CID_GEGLU_NLOOP=1", "CID_GEGLU_NLOOP=2", "CID_GEGLU_NLOOP=4", "CID_GEGLU_H32=0",
            "CID_GEMM_NBUF=2", "CID_GEMM_NBUF=3", "CID_GEMM_NOHALO=1", "CID_CONV_H32=0", "CID_CONV_H32=2", "CID_UPCONV_FOLD=0",
            "CID_XCD_2D=0")


# ----------------------------------------------------------------------------- descriptors
def blank(**kw) -> dict:
    d = dict.fromkeys(FIELDS, 0)
    d.update(x1=64, w=64, out=64, rows_per_sample=1, taps=1, stride=1)
    d.update(kw)
    return d


def from_census(rec: dict) -> dict:
    """a census record (gemm_census.DESC_FIELDS) as a grid descriptor; ``stats`` there = gn_stats attached here"""
    d = blank(**{k: rec[k] for k in gemm_census.DESC_INTS})
    d["ws_bytes"] = rec["ws_bytes"]
    for p in ("x2", "bias", "rowbias", "res", "vt", "ws", "out2", "w_up4"):
        d[p] = 64 * rec["has_" + p]
    d["ln_s"] = d["ln_b"] = 64 * rec["has_ln_s"]
    d["ln_eps_pos"] = rec["has_ln_s"]
    d["att_kp"] = d["att_vp"] = d["att_kvrow"] = 64 * rec["has_att_kp"]
    d["gn_stats"] = 64 * rec["stats"]
    return d


def linear(M, N, K, **kw) -> dict:
    return blank(M=M, N=N, c1=K, ld1=K, ldo=N // 2 if kw.get("mode") == 1 else N, ldr=N, bias=64, **kw)


def conv(B, Hi, Wi, cin, cout, up=0, stride=1, **kw) -> dict:
    Ho, Wo = (Hi << up, Wi << up) if stride == 1 else (Hi // 2, Wi // 2)
    return blank(M=B * Ho * Wo, N=cout, c1=cin, ld1=cin, ldo=cout, ldr=cout, taps=9, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, stride=stride,
                 up=up, bias=64, **kw)


def qattn(M, heads, dhead, ntok, **kw) -> dict:
    C_ = heads * dhead
    d = blank(M=M, N=C_, c1=C_, ld1=C_, ldo=C_, ldr=C_, mode=3, heads=heads, dhead=dhead, dvp=(dhead + 31) // 32 * 32, ntok=ntok,
              att_kp=64, att_vp=64, att_kvrow=64, att_n_txt=77, att_n_ip=4)
    d.update(kw)
    return d


LN_ON = dict(ln_s=64, ln_b=64, ln_eps_pos=1, bias=0)
LN_OFF = dict(ln_s=0, ln_b=0, ln_eps_pos=0, bias=64)


def synthetic() -> list:
    """[(base descriptor, [overrides, ...])]: the refusals of every argument check and the rules' edges"""
    lin, cv = linear(4096, 320, 320), conv(8, 32, 32, 640, 640, ws=64, ws_bytes=64 << 20)
    out = [(lin, [{}, dict(x1=0), dict(w=0), dict(out=0), dict(taps=3), dict(c1=48), dict(c1=96, ld1=96), dict(c2=64, ld2=64),
                  dict(c1=96, ld1=96, c2=32, ld2=32, x2=64), dict(N=0), dict(N=48), dict(M=0), dict(mode=4), dict(mode=-1),
                  dict(ld1=324), dict(ldo=324), dict(c2=320, ld2=324, x2=64), dict(res=64, ldr=324), dict(out=72), dict(res=72),
                  dict(out2=72), dict(out2=64), dict(out2=64, mode=1, N=2560, ldo=1280), dict(ln_s=64), dict(ln_b=64), LN_ON,
                  dict(LN_ON, bias=64), dict(LN_ON, ln_eps_pos=0), dict(LN_ON, c2=320, ld2=320, x2=64), dict(M=4000000),
                  dict(pad_mode=2), dict(pad_mode=1), dict(w_up4=64), dict(act=2), dict(act=1), dict(act=1, mode=1, N=2560, ldo=1280),
                  dict(act=1, gn_stats=64), dict(act=1, ws=64, ws_bytes=1 << 20), dict(LN_ON, act=1), dict(act=1, N=128, ldo=128),
                  dict(act=1, N=64, ldo=64), dict(act=1, N=96, ldo=96), dict(act=1, M=300), dict(mode=1, N=96, ldo=48),
                  dict(mode=1, N=192, ldo=96), dict(gn_stats=64), dict(gn_stats=64, N=96, ldo=96), dict(gn_stats=64, N=128, ldo=128),
                  dict(gn_stats=64, M=4100), dict(gn_stats=64, mode=1, N=2560, ldo=1280), dict(gn_stats=64, N=5120, ldo=5120),
                  dict(gn_stats=64, M=256, c1=5120, ld1=5120, ws=64, ws_bytes=64 << 20)] +
                 # mode 2 (fused QKV + transposed V)
                 [dict(dict(mode=2, N=960, n_vt0=640, ldo=640, vt=64, heads=8, dhead=40, dvp=64, ntok=4096), **kw)
                  for kw in ({}, dict(vt=0), dict(ntok=4100), dict(ntok=1000), dict(n_vt0=600), dict(dvp=32), dict(heads=0), LN_ON,
                             dict(M=32768), dict(M=8192, ntok=1024), dict(M=2048, ntok=256))]),
           (cv, [{}, dict(act=1, ws=0, ws_bytes=0), dict(Hi=0), dict(stride=3), dict(up=2), dict(M=8 * 1024 + 64),
                 dict(LN_ON), dict(pad_mode=1), dict(w_up4=64), dict(gn_stats=64), dict(gn_stats=64, c1=1280, ld1=1280),
                 dict(rowbias=64, ld_rowbias=640, rows_per_sample=1024), dict(rowbias=64, ld_rowbias=640, rows_per_sample=1000),
                 dict(res=64), dict(out2=64), dict(c1=320, ld1=320, c2=320, ld2=320, x2=64)])]
    # pad_mode 1 (Downsample2D(padding=0)): legal, and each condition broken
    pad = conv(1, 64, 64, 128, 128, stride=2, pad_mode=1, ws=64, ws_bytes=16 << 20)
    out.append((pad, [{}, dict(mode=1), dict(stride=1), dict(up=1), dict(Hi=63), dict(Wi=62), dict(Ho=31, M=31 * 32), dict(ws=0),
                      dict(N=320, ldo=320, c1=320, ld1=320), dict(M=8 * 1024)]))
    # w_up4 (Upsample2D from folded weights): legal at several sizes, and each condition broken
    up4 = conv(8, 32, 32, 640, 640, up=1, w_up4=64, ws=64, ws_bytes=64 << 20)
    out.append((up4, [{}, dict(w_up4=72), dict(up=0, Ho=32, Wo=32, M=8192), dict(mode=1), dict(res=64), dict(rowbias=64, ld_rowbias=640,
                      rows_per_sample=4096), dict(c1=320, ld1=320, c2=320, ld2=320, x2=64), dict(N=128, ldo=128), dict(gn_stats=64)] +
                     [dict(M=B * 4 * s * s, Hi=s, Wi=s, Ho=2 * s, Wo=2 * s, c1=c, ld1=c, N=c, ldo=c)
                      for B, s, c in ((8, 8, 1280), (8, 16, 1280), (2, 16, 1280), (1, 32, 640), (2, 64, 320), (4, 64, 320), (2, 24, 640),
                                      (8, 48, 320), (2, 128, 320))]))
    # image sizes on and off the whole-row rule of the halo / conv3x3.hip tiles, with and without a split-K workspace
    sizes = [dict(M=B * h * w, Hi=h, Wi=w, Ho=h, Wo=w, c1=ci, ld1=ci, N=co, ldo=co, ws=ws, ws_bytes=(64 << 20) * (ws > 0))
             for B, h, w in ((1, 8, 8), (8, 8, 8), (2, 16, 16), (8, 16, 16), (1, 32, 32), (2, 32, 32), (1, 64, 64), (2, 64, 64), (8, 64, 64),
                             (2, 128, 128), (2, 64, 96), (2, 96, 64), (8, 48, 48), (8, 24, 24), (8, 40, 40), (4, 12, 12), (2, 108, 144),
                             (1, 256, 256), (2, 20, 64))
             for ci, co in ((320, 320), (640, 640), (1280, 1280), (1280, 640), (2560, 1280), (128, 128), (512, 256))
             for ws in (64, 0)]
    out.append((cv, sizes[::2] + [dict(s, up=1, Ho=2 * s["Ho"], Wo=2 * s["Wo"], M=4 * s["M"]) for s in sizes[1::7]]
                + [dict(s, stride=2, Ho=s["Ho"] // 2, Wo=s["Wo"] // 2, M=s["M"] // 4) for s in sizes[3::7]]))
    # mode 3 at each head width (and one the kernel has no instance for), with and without the LayerNorm fold
    q = qattn(8192, 8, 80, 1024)
    m3 = [dict(qattn(M, h, dh, ntok), **ln) for ln in ({}, dict(ln_s=64, ln_b=64, ln_eps_pos=1))
          for M, h, dh, ntok in ((32768, 8, 40, 4096), (32768, 5, 64, 4096), (8192, 10, 64, 1024), (8192, 8, 80, 1024),
                                 (2048, 16, 80, 256), (512, 16, 80, 64), (16384, 10, 64, 4096), (4096, 20, 64, 1024),
                                 (1024, 8, 160, 256), (2048, 8, 160, 1024), (32768, 2, 160, 4096), (8192, 8, 96, 1024),
                                 (8192, 10, 64, 192), (8192, 8, 80, 192), (65536, 8, 80, 4096), (8192, 8, 80, 1000))]
    out.append((q, m3 + [dict(att_kp=0), dict(att_kvrow=0), dict(bias=64), dict(res=64), dict(gn_stats=64), dict(heads=4), dict(att_n_txt=76),
                         dict(att_n_ip=8), dict(ntok=0), dict(M=8200), dict(taps=9, Hi=32, Wi=32, Ho=32, Wo=32), dict(act=1)]))
    # GEGLU projections around the linear_h32 rule (K >= 1024, M % 256 == 0, >= 256 tiles of 256 x 160), plain and LN-folded
    g = linear(4096, 10240, 1280, mode=1)
    out.append((g, [dict(M=M, N=8 * c, c1=c, ld1=c, ldo=4 * c, ldr=8 * c, **ln) for ln in (LN_OFF, LN_ON)
                    for c in (320, 640, 960, 1024, 1280, 1600, 1920, 2560)
                    for M in (256, 512, 768, 1024, 1152, 1280, 2048, 4096, 8192, 16384, 32768)]))
    return out


def neighbours_of(idx: int, rec: dict, plan: dict) -> list:
    """overrides around one census descriptor: M one tile off in both directions (twice / half the samples for a convolution,
    whose M must stay whole images), the workspace absent or too small to split, the LayerNorm fold toggled, statistics asked"""
    d, bm, out = from_census(rec), plan["bm"], []
    out += [dict(M=d["M"] + bm)] + ([dict(M=d["M"] - bm)] if d["M"] > bm else [])
    if d["taps"] == 9 or d["mode"] >= 2:
        out += [dict(M=2 * d["M"])] + ([dict(M=d["M"] // 2)] if d["M"] % 2 == 0 else [])
    if d["ws"]:
        out += [dict(ws=0, ws_bytes=0), dict(ws_bytes=4 * d["M"] * d["N"]), dict(ws_bytes=8 * d["M"] * d["N"])]
    if d["taps"] == 1 and d["c2"] == 0:
        out.append(dict(LN_OFF) if d["ln_s"] else dict(LN_ON))
    if d["mode"] == 0 and not d["gn_stats"]:
        out.append(dict(gn_stats=64))
    return [[idx, o] for o in out]


def build_cases():
    """-> (descs, neighbours): the census records (all of them), neighbours of one record per launch variant, the synthetic set"""
    fixture = gemm_census.load()
    seen, descs, index = set(), [], {}
    for rec, plan in gemm_census.all_records(fixture):
        row = tuple(from_census(rec).values())
        if row not in seen:
            seen.add(row)
            index[row] = len(descs)
            descs.append(list(row))
    nb = []
    for key, (rec, plan) in gemm_census.keys_of(gemm_census.all_records(fixture)).items():
        nb += neighbours_of(index[tuple(from_census(rec).values())], rec, plan)
    for base, overrides in synthetic():
        descs.append(list(base.values()))
        nb += [[len(descs) - 1, o] for o in overrides]
    return descs, nb


def expand(descs, neighbours) -> list:
    cases = [dict(zip(FIELDS, row)) for row in descs]
    return cases + [dict(cases[i], **o) for i, o in neighbours]


# ----------------------------------------------------------------------------- planning (in a process of the setting's own)
def plan_cases(cases) -> list:
    from consistentid_amd import _lib
    lib = _lib.load()
    out = []
    for c in cases:
        d, info = _lib.GemmDesc(), _lib.GemmPlanInfo()
        for f in FIELDS:
            if f != "ln_eps_pos":
                setattr(d, f, c[f] or None if f in PTRS else c[f])
        d.ln_eps, d.att_ip_scale = (1e-5 if c["ln_eps_pos"] else 0.0), 1.0
        rc = lib.cid_gemm_plan(C.byref(d), C.byref(info))
        out.append([rc, lib.cid_last_error().decode()] if rc else [0] + [int(getattr(info, f)) for f in INFO_FIELDS])
    return out


def child_env(setting: str = "") -> dict:
    """the environment without any CID_* switch (CID_LIBRARY stays), plus ``setting`` ("NAME=VALUE" or "")"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CID_") or k == "CID_LIBRARY"}
    if setting:
        name, value = setting.split("=")
        env[name] = value
    return env


def run_child(what: str, path, setting: str = ""):
    """``python tests/gemm_plan_grid.py <what> <path>`` under ``setting`` -> its JSON answer"""
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), what, str(path)], env=child_env(setting), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, f"{what} under {setting or 'the defaults'} failed:\n{r.stderr[-2000:]}"
    return json.loads(r.stdout.splitlines()[-1])


# ----------------------------------------------------------------------------- the fixture
def load(path=GOLDEN) -> dict:
    z = json.loads(Path(path).read_text())
    assert tuple(z["fields"]) == FIELDS and tuple(z["info_fields"]) == INFO_FIELDS, \
        f"{path} was written for other fields: regenerate it ({REGENERATE})"
    return z


def expected(z: dict, setting: str) -> list:
    want = list(z["default"])
    for i, k in z["settings"].get(setting, []):
        want[i] = k
    return [z["results"][k] for k in want]


def dump(descs, neighbours, default, settings, path):
    """``default``: one result per case; ``settings``: {setting: one result per case}"""
    results, number = [], {}

    def k_of(r):
        key = json.dumps(r)
        if key not in number:
            number[key] = len(results)
            results.append(r)
        return number[key]

    d0 = [k_of(r) for r in default]
    per = {s: [[i, k_of(r)] for i, r in enumerate(got) if k_of(r) != d0[i]] for s, got in settings.items()}
    rows = lambda xs: "[\n" + ",\n".join("  " + json.dumps(x, separators=(",", ":")) for x in xs) + "\n ]"
    flat = lambda xs: json.dumps(xs, separators=(",", ":"))
    sets = ",\n".join(f"  {json.dumps(s)}: {flat(diff)}" for s, diff in per.items())
    Path(path).write_text("{\n" + f' "fields": {json.dumps(list(FIELDS))},\n "info_fields": {json.dumps(list(INFO_FIELDS))},\n'
                          f' "descs": {rows(descs)},\n "neighbours": {rows(neighbours)},\n "results": {rows(results)},\n'
                          f' "default": {flat(d0)},\n "settings": {{\n' + sets + "\n }\n}\n")


if __name__ == "__main__":      # the child: plan / fold <file> -> one JSON line
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    what, path = sys.argv[1], Path(sys.argv[2])
    z = json.loads(path.read_text())
    if what == "plan":
        print(json.dumps(plan_cases(expand(z["descs"], z["neighbours"])), separators=(",", ":")))
    elif what == "fold":      # [[M, C_], ...] -> ops.ln_fold_geglu of each
        from consistentid_amd import ops
        print(json.dumps([int(ops.ln_fold_geglu(M, C_)) for M, C_ in z]))
    else:
        raise SystemExit(f"unknown request {what}")
