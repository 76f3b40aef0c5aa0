"""Launch paths of the transformer block (test helper, not a conftest).

``HipUNet._transformer`` and ``HipUNet.cross_attention`` decide per level and per launch which kernels run, on which
buffers and at which pitches, from ``(channels, heads, context, B, Bp, H, W)``.  A *combination* is what they decide:

    (pad, dedup, qkv, xattn, tail, geglu, stats)        -- FIELDS

``predict`` evaluates the host predicates of ``ops`` / ``unet`` (no GPU, no launch); ``Trace`` records what a block really
launched and ``observed`` reads the same fields off that record.  The two share the field names and nothing else.

tests/golden/transformer_paths.json files one shape under every combination the three model families reach on GRID (the
smallest ``B * Np * c`` that has it; tests/golden/make_golden_transformer_paths.py writes it, no GPU needed).
tests/test_transformer_paths_host.py checks the table against the predicates, tests/test_gpu_transformer_paths.py runs one
parity case per row.

Contexts past ``ops.XATTN_SHORT_MAX`` = 96 rows (``LONG_CONTEXT``, ``CAP_CONTEXT``) take the long-context core in every layer
(``xattn`` = "long+fold" / "long"), pad the token axis to 64 at every width and fold the tail wherever ``ops.ff2_fold`` holds.
Their rows stand under "long" in the same file, one per ``LONG_KEY`` -- the fields such a context changes (``enumerate_long``) --
and one per family at 1024 text rows (``cap_shape``); the rows under "cases" are those of the default context, unchanged."""
import contextlib
import json
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden" / "transformer_paths.json"
REGENERATE = "python tests/golden/make_golden_transformer_paths.py   (no GPU needed; writes tests/golden/transformer_paths.json)"

FIELDS = ("pad", "dedup", "qkv", "xattn", "tail", "geglu", "stats")
SHAPE = ("c", "heads", "n_layers", "n_txt", "n_ip", "B", "Bp", "H", "W")
QKV = ("fold", "ln+gemm")
XATTN = ("gen3", "gen1", "qattn+fold", "qattn", "core+fold", "core", "long+fold", "long")
TAIL = ("folded", "ff2+proj_out")
GEGLU = ("fold", "ln+h32", "ln+gemm")

# the environment switches the predicates read at import, with the value each has when it is not set
SWITCHES = {"CID_LN_FOLD": "auto", "CID_FF2_FOLD": "auto", "CID_GEGLU_FOLD_MAX": "8192", "CID_QATTN_LNFOLD_MAX": "8192",
            "CID_XATTN_FUSED_MAX_C": "320", "CID_QATTN": "1", "CID_XATTN_GEN": "3", "CID_XATTN_V2": "1", "CID_CFG_DEDUP": "1"}

MAX_TOKENS = 21000      # tokens of a case, B * H * W: what its fp32 CPU oracle computes on (a few seconds at the most)

# ----------------------------------------------------------------------------- the grid
BATCHES = ((1, 1), (2, 1), (2, 2), (3, 3), (4, 2), (4, 4), (6, 3), (8, 4), (16, 8), (32, 16))       # (B, Bp): CFG batch, distinct samples
SIZES = tuple((s, s) for s in (32, 40, 48, 56, 64, 72, 80, 96, 128)) + ((64, 96), (96, 64), (40, 64), (88, 64), (120, 64), (24, 40),
                                                                        (104, 72))                 # latent H x W
GRID = tuple((B, Bp, H, W) for B, Bp in BATCHES for H, W in SIZES)

# what ran at the models' real widths against the oracle before these tests: the forwards and trajectories of
# tests/test_gpu_fullsize.py, test_gpu_controlnet.py::test_sd15_controlnet_forward_full_size and the workloads of
# gemm_census.record_census, as (B, Bp, H, W) of the latents
COVERED_BEFORE = {
    "sd15": ((2, 2, 64, 64), (2, 2, 64, 96), (8, 8, 64, 64), (4, 4, 64, 64), (8, 4, 64, 64), (16, 8, 64, 64), (2, 1, 64, 64),
             (2, 1, 64, 96)),
    "sdxl": ((2, 2, 128, 128), (4, 4, 128, 128), (2, 2, 144, 108)),
    "controlnet": ((1, 1, 64, 64), (2, 2, 64, 64), (8, 8, 64, 64)),
}
# SDXL's ten layers at 1280 channels are two here (only the last layer's tail differs from the others)
TEST_LAYERS = 2


FAMILIES = ("sd15", "sdxl", "controlnet")
CONTEXT = {"sd15": (77, 4), "sdxl": (77, 4), "controlnet": (81, 0)}             # (n_txt, n_ip) of the default prompt
# contexts past ops.XATTN_SHORT_MAX rows (csrc/xattn_long.hip): two and three 77-row chunks, and the most rows a pipeline takes
# (1024 text rows + the ID rows).  The ControlNet is handed text and ID rows as ONE text stream: 154 + 4 and 1024 + 4 rows
LONG_CONTEXT = {"sd15": (154, 4), "sdxl": (231, 4), "controlnet": (158, 0)}
CAP_CONTEXT = {"sd15": (1024, 4), "sdxl": (1024, 4), "controlnet": (1028, 0)}
CAP_CHANNELS = 1280
LONG_KEY = ("c", "heads", "pad", "dedup", "xattn", "tail")      # what a long row is filed under: see enumerate_long


def family_config(family: str, context=None):
    """the product's UNetConfig of a family and its context layout (n_txt, n_ip): ``context``, or the default prompt's"""
    from consistentid_amd import unet_spec
    cfg = unet_spec.sdxl_config() if family == "sdxl" else unet_spec.sd15_config()
    return (cfg,) + tuple(CONTEXT[family] if context is None else context)


def levels(family: str, B: int, Bp: int, H: int, W: int, context=None):
    """every transformer the family's model runs on a (B, Bp) batch of H x W latents, in execution order, as SHAPE tuples.
    Only SD1.5's first transformer sees the Bp distinct samples of a CFG batch (HipUNet.forward_tokens: a shared timestep
    row, and the first down block has attention); the ControlNet is the encoder half."""
    from consistentid_amd import unet_spec
    cfg, n_txt, n_ip = family_config(family, context)
    downs, mid, ups = unet_spec.walk(cfg)
    out, first = [], family == "sd15"
    for blk in downs:
        for t in blk.attentions:
            out.append((t.channels, t.heads, min(t.n_layers, TEST_LAYERS), n_txt, n_ip, B, Bp if first else B, H, W))
            first = False
        first = False
        if blk.sampler:
            H, W = H // 2, W // 2
    t = mid.attentions[0]
    out.append((t.channels, t.heads, min(t.n_layers, TEST_LAYERS), n_txt, n_ip, B, B, H, W))
    for blk in ([] if family == "controlnet" else ups):
        for t in blk.attentions:
            out.append((t.channels, t.heads, min(t.n_layers, TEST_LAYERS), n_txt, n_ip, B, B, H, W))
        if blk.sampler:
            H, W = H * 2, W * 2
    return out


# ----------------------------------------------------------------------------- prediction (host predicates only)
def long_context(n_txt, n_ip) -> bool:
    """more context rows than the register-resident cross-attention kernels hold: every layer runs csrc/xattn_long.hip"""
    from consistentid_amd import ops
    return n_txt + n_ip > ops.XATTN_SHORT_MAX


def padded_tokens(c, heads, n_txt, n_ip, H, W) -> int:
    """tokens per sample after HipUNet._transformer's zero-padding of the token axis"""
    from consistentid_amd import ops
    if long_context(n_txt, n_ip):       # the long core tiles 32 tokens: the self-attention's 64 decide
        return -(-H * W // 64) * 64
    gen3 = ops.xattn_generation() >= 3 and ops.id_xattn3_supported(c, heads, n_txt, n_ip)
    need = 128 if (128 < c <= int(SWITCHES["CID_XATTN_FUSED_MAX_C"]) and not gen3) else 64
    return -(-H * W // need) * need


def predict(c, heads, n_layers, n_txt, n_ip, B, Bp, H, W) -> tuple:
    """the combination (FIELDS) ``HipUNet._transformer`` takes for this block, from the predicates of ``ops`` / ``unet``"""
    from consistentid_amd import ops, unet
    assert n_layers >= 1 and B % Bp == 0
    Np = padded_tokens(c, heads, n_txt, n_ip, H, W)
    pad = Np != H * W
    M1, M = Bp * Np, B * Np         # rows up to the self-attention / from the cross-attention on
    qkv = "fold" if ops.ln_fold(M1) else "ln+gemm"
    long = long_context(n_txt, n_ip)
    gen3 = not long and ops.xattn_generation() >= 3 and ops.id_xattn3_supported(c, heads, n_txt, n_ip)
    gen1 = not long and unet.fused_gen1(c, M)
    if long:
        xattn = "long+fold" if ops.ln_fold(M) else "long"
    elif gen3:
        xattn = "gen3"
    elif gen1:
        xattn = "gen1"
    elif ops.qattn_supported(c, heads, Np, n_txt, n_ip):
        xattn = "qattn+fold" if ops.ln_fold_q(M) else "qattn"
    else:
        xattn = "core+fold" if ops.ln_fold(M) else "core"
    gn_hw = 0 if pad else Np
    tail = "folded" if ops.ff2_fold(M, c, gn_hw) and (long or gen3 or not gen1) else "ff2+proj_out"
    if ops.ln_fold_geglu(M, c):
        geglu = "fold"
    else:
        geglu = "ln+h32" if ops._geglu_on_h32(M, c) else "ln+gemm"
    return (pad, Bp != B, qkv, xattn, tail, geglu, gn_hw > 0)


# ----------------------------------------------------------------------------- observation (what a block launched)
class Trace:
    """``with Trace(B, Bp, H, W) as tr: ...`` -- tr.records: one dict per launch of the ``ops`` entry points the transformer
    block calls (every caller goes through the module attribute), in order: its name and the keywords that tell the paths
    apart.  ``tr.only(engine, name)`` restricts the record to the transformer called ``name`` and keeps that call's input
    and output in ``tr.block_in`` / ``tr.block_out``."""
    OPS = ("gemm", "layernorm", "self_attn", "id_xattn", "id_xattn3", "id_xattn_core", "id_xattn_long")
    INTS = ("M", "N", "c1", "ld1", "ldo", "mode", "ntok", "n_keys", "gn_hw", "ldx", "B", "C_")
    HAS = ("ln", "att", "out2", "res")

    def __init__(self, B, Bp, H, W):
        self.shape = (B, Bp, H, W)
        self.records = []
        self.active = True
        self.block_in = self.block_out = None

    def _wrap(self, name, fn):
        from consistentid_amd import ops

        def call(*a, **kw):
            if self.active:
                rec = {"op": name, "mode": 0, "ntok": 0, "gn_hw": 0} if name == "gemm" else {"op": name}
                rec.update({k: (0 if kw.get(k) is None else int(kw[k])) for k in self.INTS if k in kw})
                rec.update({k: kw.get(k) is not None for k in self.HAS})
                if name == "gemm":
                    rec["family"] = ops.gemm_plan(*a, **kw)["family"]
                self.records.append(rec)
            return fn(*a, **kw)
        return call

    def __enter__(self):
        from consistentid_amd import ops
        self._ops, self._orig = ops, {n: getattr(ops, n) for n in self.OPS}
        for n, fn in self._orig.items():
            setattr(ops, n, self._wrap(n, fn))
        return self

    def __exit__(self, *exc):
        for n, fn in self._orig.items():
            setattr(self._ops, n, fn)
        return False

    @contextlib.contextmanager
    def only(self, engine, name):
        inner, self.active = engine._transformer, False

        def transformer(t, x, *a, **kw):
            if t.name != name:
                return inner(t, x, *a, **kw)
            self.active, self.block_in = True, x
            try:
                self.block_out = inner(t, x, *a, **kw)
            finally:
                self.active = False
            return self.block_out
        engine._transformer = transformer
        try:
            yield self
        finally:
            del engine._transformer         # the instance attribute: the class's method shows again


def _one(values, what):
    """the value every layer of the block agrees on"""
    got = sorted(set(values), key=str)
    return got[0] if len(got) == 1 else f"{what}: {got}"


def observed(trace) -> tuple:
    """the combination (FIELDS) read off the launches of one transformer block"""
    B, Bp, H, W = trace.shape
    rs = trace.records
    before = lambda i, op: i > 0 and rs[i - 1]["op"] == op
    qkv, xattn, geglu = [], [], []
    for i, r in enumerate(rs):
        if r["op"] == "gemm" and r["mode"] == 2:
            qkv.append("fold" if r["ln"] else ("ln+gemm" if before(i, "layernorm") else "gemm without norm1"))
        elif r["op"] == "gemm" and r["mode"] == 1:
            if r["ln"]:
                geglu.append("fold")
            elif not before(i, "layernorm"):
                geglu.append("gemm without norm3")
            else:
                geglu.append("ln+h32" if r["family"] == "geglu_h32" else "ln+gemm")
        elif r["op"] == "gemm" and r["mode"] == 3:
            xattn.append("qattn+fold" if r["ln"] else ("qattn" if before(i, "layernorm") else "qattn without norm2"))
        elif r["op"] == "id_xattn3":
            xattn.append("gen3")
        elif r["op"] == "id_xattn":
            xattn.append("gen1")
        elif r["op"] in ("id_xattn_core", "id_xattn_long"):
            name = "core" if r["op"] == "id_xattn_core" else "long"
            q = rs[i - 1] if before(i, "gemm") else {"ln": False, "mode": -1}
            if q["mode"] != 0:
                xattn.append(f"{name} without q")
            else:
                xattn.append(f"{name}+fold" if q["ln"] else (name if before(i - 1, "layernorm") else f"{name} without norm2"))
    first = next(r for r in rs if r["op"] == "gemm" and r["mode"] == 2)
    keys = _one([(r["N"], r["n_keys"]) for r in rs if r["op"] == "self_attn"], "self_attn")
    ntok = _one([r["ntok"] for r in rs if r["op"] == "gemm" and r["mode"] in (2, 3)], "ntok")
    pad = ntok != H * W
    if keys != (ntok, H * W):
        pad = f"self_attn on {keys}, projections on {ntok} tokens of {H * W}"
    gemms = [r for r in rs if r["op"] == "gemm"]
    tail = "folded" if any(r["mode"] == 0 and r["c1"] == 5 * r["N"] for r in gemms) else "ff2+proj_out"
    return (pad, first["M"] == Bp * ntok and first["M"] != B * ntok, _one(qkv, "qkv"), _one(xattn, "xattn"), tail,
            _one(geglu, "geglu"), gemms[-1].get("gn_hw", 0) > 0)


# ----------------------------------------------------------------------------- the table
def enumerate_grid(family: str, shapes=GRID) -> dict:
    """{(c,) + combination: the smallest SHAPE that has it} over every level of the family's model on ``shapes``; the size is
    ``B * Np * c``, ties broken by the integers.  Shapes above MAX_TOKENS tokens are kept apart: {key: None} where
    no shape within the bound has the combination."""
    best = {}
    for B, Bp, H, W in shapes:
        for shp in levels(family, B, Bp, H, W):
            c, heads, _, n_txt, n_ip, b, bp, h, w = shp
            tokens = b * padded_tokens(c, heads, n_txt, n_ip, h, w)
            key = (c,) + predict(*shp)
            if b * h * w > MAX_TOKENS:
                best.setdefault(key, None)
                continue
            size = (tokens * c, shp)
            if best.get(key) is None or size < best[key]:
                best[key] = size
    return {k: (None if v is None else v[1]) for k, v in sorted(best.items(), key=lambda kv: str(kv[0]))}


def combinations_of(family: str, shapes) -> set:
    return {(shp[0],) + predict(*shp) for s in shapes for shp in levels(family, *s)}


def long_key(shp) -> tuple:
    """(c, heads, pad, dedup, xattn, tail) of a SHAPE: LONG_KEY"""
    pad, dedup, _, xattn, tail, _, _ = predict(*shp)
    return (shp[0], shp[1], pad, dedup, xattn, tail)


def enumerate_long(family: str, shapes=GRID) -> dict:
    """{LONG_KEY tuple: the smallest SHAPE that has it} under the family's LONG_CONTEXT within MAX_TOKENS tokens, sized and
    tie-broken as in ``enumerate_grid``.  A long context changes the cross-attention, the padding rule and the tail's
    condition only; ``qkv``, ``geglu`` and ``stats`` are decided as at 77 rows, where every value has a row, so they are no
    part of the key.  The ControlNet runs the same ``_transformer``: of its keys only the smallest shape per width stays."""
    best = {}
    for B, Bp, H, W in shapes:
        for shp in levels(family, B, Bp, H, W, LONG_CONTEXT[family]):
            c, heads, _, n_txt, n_ip, b, bp, h, w = shp
            if b * h * w > MAX_TOKENS:
                continue
            size = (b * padded_tokens(c, heads, n_txt, n_ip, h, w) * c, shp)
            key = long_key(shp)
            if key not in best or size < best[key]:
                best[key] = size
    if family == "controlnet":
        per_width = {}
        for key, size in best.items():
            if key[0] not in per_width or size < per_width[key[0]][1]:
                per_width[key[0]] = (key, size)
        best = dict(per_width.values())
    return {k: v[1] for k, v in sorted(best.items(), key=lambda kv: str(kv[0]))}


def cap_shape(family: str, shapes=GRID) -> tuple:
    """the smallest SHAPE of a CAP_CHANNELS-wide level under the family's CAP_CONTEXT"""
    sized = [(shp[5] * padded_tokens(shp[0], shp[1], shp[3], shp[4], shp[7], shp[8]) * shp[0], shp) for s in shapes
             for shp in levels(family, *s, CAP_CONTEXT[family]) if shp[0] == CAP_CHANNELS and shp[5] * shp[7] * shp[8] <= MAX_TOKENS]
    return min(sized)[1]


def load(path=GOLDEN) -> dict:
    """-> {"cases": {family: [(SHAPE tuple, combination tuple), ...]}, "omitted": {family: [(c, combination, reason), ...]},
    "long": {family: [(SHAPE tuple, combination tuple), ...]}}: "cases" at the default context, "long" under LONG_CONTEXT and
    (the last row of a family) CAP_CONTEXT"""
    z = json.loads(Path(path).read_text())
    assert tuple(z["shape"]) == SHAPE and tuple(z["fields"]) == FIELDS, f"{path} was written for other fields: {REGENERATE}"
    n = len(SHAPE)
    rows = lambda d: {f: [(tuple(r[:n]), tuple(r[n:])) for r in rs] for f, rs in d.items()}
    return {"cases": rows(z["cases"]), "long": rows(z["long"]),
            "omitted": {f: [(r[0], tuple(r[1:1 + len(FIELDS)]), r[-1]) for r in rows] for f, rows in z["omitted"].items()}}


def dump(cases: dict, omitted: dict, long: dict, path):
    """``cases``: {family: {(c,) + combination: SHAPE}}; ``omitted``: {family: [((c,) + combination, reason), ...]};
    ``long``: {family: [SHAPE, ...]} (filed under ``predict`` of each)"""
    row = lambda r: "   " + json.dumps(list(r), separators=(",", ":"))
    block = lambda d: ",\n".join(f"  {json.dumps(f)}: [\n" + ",\n".join(row(r) for r in rows) + "\n  ]" for f, rows in d.items())
    c = {f: sorted((list(shp) + list(key[1:]) for key, shp in d.items()), key=lambda r: r[:len(SHAPE)]) for f, d in cases.items()}
    o = {f: [list(key) + [reason] for key, reason in rows] for f, rows in omitted.items()}
    lg = {f: [list(shp) + list(predict(*shp)) for shp in sorted(shapes)] for f, shapes in long.items()}
    Path(path).write_text("{\n" + f' "shape": {json.dumps(list(SHAPE))},\n "fields": {json.dumps(list(FIELDS))},\n'
                          + ' "cases": {\n' + block(c) + '\n },\n "omitted": {\n' + block(o) + '\n },\n "long": {\n' + block(lg)
                          + "\n }\n}\n")


def case_id(family, shp) -> str:
    c, heads, n_layers, n_txt, n_ip, B, Bp, H, W = shp
    ctx = "" if (n_txt, n_ip) == CONTEXT[family] else f"-ctx{n_txt}+{n_ip}"
    return f"{family}-c{c}-B{B}" + (f"of{Bp}" if Bp != B else "") + f"-{H}x{W}" + ctx


def ordered_cases(table) -> list:
    """[(family, SHAPE, combination)]: family by family, width by width, a width's long rows behind its short rows -- one
    engine per (family, width) serves them in turn and crosses 81, 158 and 1028 context rows"""
    out = []
    for f in table["cases"]:
        rows = [(shp[0], long_context(shp[3], shp[4]), shp, comb) for shp, comb in table["cases"][f] + table["long"].get(f, [])]
        out += [(f, shp, comb) for _, _, shp, comb in sorted(rows, key=lambda r: r[:3])]
    return out
