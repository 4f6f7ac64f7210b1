"""Which refusal wins: return code, exact ecamd_last_error() text and untouched memory for every entry
point of ecamd_check.hip, ecamd_decode_masks.hip and ecamd_xor_decode_masks.hip.

Every case calls one entry point with one or two faulty arguments on two stripes of 64-byte fragments,
every result array filled with a canary, and asserts the code, the text, and that no result word, no
host result and no fragment byte changed.  The double faults pin the ORDER of the validations: which
of two refusals a caller sees.  An empty batch (nstripes == 0) returns 0, moves no launch counter and
still writes `checked` / `covered`.  The texts are the ones the library gave before its check driver
was restructured; a change of any of them is a change of behaviour.
"""
import ctypes as C

import numpy as np
import pytest

from liberasurecode_amd import _lib
from liberasurecode_amd import device as D

pytestmark = pytest.mark.gpu

EINVAL = -22
BS, S, NFRAGS = 64, 2, 14
CANARY = 0xA5A5A5A5
ICANARY = CANARY - (1 << 32)

LAYOUT = ("base", "stripe_stride", "frag_stride", "blocksize", "nstripes")
RS, XOR, DEG = ("k", "m", "missing"), ("k", "m", "hd"), ("k", "m", "hd", "missing")
N3, N4 = ("n0", "n1", "n2"), ("n0", "n1", "n2", "n3")
ENTRY = {
    "ecamd_rs_check": RS + LAYOUT + ("status", "checked", "stream"),
    "ecamd_rs_locate": RS + LAYOUT + ("status", "suspects", "checked", "stream"),
    "ecamd_rs_locate_pairs": RS + LAYOUT + ("status", "suspects", "pairs", "checked", "stream"),
    "ecamd_rs_correct": RS + LAYOUT + ("status", "suspects", "pairs", "counts", "checked", "stream"),
    "ecamd_rs_scrub": ("k", "m") + LAYOUT + ("status", "suspects") + N3 + ("stream",),
    "ecamd_rs_scrub_pairs": ("k", "m") + LAYOUT + ("status", "suspects", "pairs") + N4 + ("stream",),
    "ecamd_xor_check": XOR + LAYOUT + ("status", "stream"),
    "ecamd_xor_locate": XOR + LAYOUT + ("status", "suspects", "stream"),
    "ecamd_xor_correct": XOR + LAYOUT + ("status", "suspects", "counts", "stream"),
    "ecamd_xor_scrub": XOR + LAYOUT + ("status", "suspects") + N3 + ("stream",),
    "ecamd_xor_check_degraded": DEG + LAYOUT + ("status", "covered", "stream"),
    "ecamd_xor_locate_degraded": DEG + LAYOUT + ("status", "suspects", "covered", "stream"),
    "ecamd_xor_correct_degraded": DEG + LAYOUT + ("status", "suspects", "counts", "covered", "stream"),
    "ecamd_rs_decode_masks": ("k", "m", "lost", "flag") + LAYOUT + ("result", "counts", "stream"),
    "ecamd_xor_decode_masks": ("k", "m", "hd", "lost", "flag") + LAYOUT + ("result", "counts", "stream"),
}
RS_ENTRIES = [e for e in ENTRY if e.startswith("ecamd_rs_") and e != "ecamd_rs_decode_masks"]
RS_MISSING = [e for e in RS_ENTRIES if "missing" in ENTRY[e]]
XOR_FULL = ["ecamd_xor_check", "ecamd_xor_locate", "ecamd_xor_correct", "ecamd_xor_scrub"]
XOR_DEG = ["ecamd_xor_check_degraded", "ecamd_xor_locate_degraded", "ecamd_xor_correct_degraded"]
MASKS = ["ecamd_rs_decode_masks", "ecamd_xor_decode_masks"]
LOCATES = [e for e in ENTRY if "suspects" in ENTRY[e]]
COUNTERS = ("ecamd_correct_launches", "ecamd_locate_pairs_launches", "ecamd_check_fused_launches",
            "ecamd_locate_fused_launches", "ecamd_xor_check_fused_launches", "ecamd_xor_locate_fused_launches",
            "ecamd_decode_masks_launches", "ecamd_xor_decode_masks_launches")

# the device words behind the result arguments (offsets in 32-bit words); `lost` is an input
WORDS = {"status": 0, "suspects": 2, "pairs": 4, "counts": 6, "result": 10, "lost": 12}
NWORDS = 16


class Ctx:
    def __init__(self):
        self.frags = D.DeviceBuffer(NFRAGS * BS * S)
        self.words = D.DeviceBuffer(4 * NWORDS)
        self.frag_image = (np.arange(NFRAGS * BS * S, dtype=np.uint32) * 131 + 7).astype(np.uint8)
        self.word_image = np.full(NWORDS, CANARY, dtype=np.uint32)
        self.word_image[WORDS["lost"]:WORDS["lost"] + 2] = (1, 2)
        self.frags.upload(self.frag_image)
        self.words.upload(self.word_image)

    def args(self, entry, over):
        """The argument values of `entry`, valid but for `over`, and the host results among them."""
        rs = entry.startswith("ecamd_rs_")
        k, m = (10, 4) if entry == "ecamd_rs_scrub_pairs" else (4, 2) if rs else (3, 3)  # a pair repair needs m >= 4
        v = {"k": k, "m": m, "hd": 3, "flag": 1, "stream": None,
             "missing": [] if rs else [1],
             "base": self.frags.ptr, "stripe_stride": NFRAGS * BS, "frag_stride": BS, "blocksize": BS, "nstripes": S}
        v.update({name: self.words.ptr + 4 * at for name, at in WORDS.items()})
        v.update(over)
        if v["missing"] is not None:
            v["missing"] = _lib.ints(list(v["missing"]) + [-1])
        host = {}
        for name in ENTRY[entry]:
            if name in ("checked", "covered"):
                host[name] = C.c_uint32(CANARY)
            elif name in N4:
                host[name] = C.c_int(ICANARY)
        return [C.byref(host[name]) if name in host else v[name] for name in ENTRY[entry]], host

    def call(self, entry, over):
        argv, host = self.args(entry, over)
        rc = getattr(_lib.dev(), entry)(*argv)
        return rc, {name: h.value for name, h in host.items()}

    def untouched(self):
        assert (self.words.download().view(np.uint32) == self.word_image).all(), "a result word changed"
        assert (self.frags.download() == self.frag_image).all(), "a fragment byte changed"


@pytest.fixture(scope="module")
def ctx():
    assert D.available(), "no HIP device"
    c = Ctx()
    yield c
    c.frags.free()
    c.words.free()


T_LAYOUT = "bad base / status / blocksize / strides"
T_MASKS_LAYOUT = "bad masks / base / blocksize / strides"
T_ALIGN = "fragment addresses must be 16-byte aligned"
T_ODD = "locate needs an even blocksize (63)"
T_MISSING = "too many missing fragments (3 > m=2)"
T_XOR_CODE = "not a flat_xor_hd code: k=3 m=3 hd=5"
T_DEG_CODE = "not a flat_xor_hd code (k=3 m=3 hd=%d) or a bad list of missing fragments"
BIG = {"k": 30, "m": 4}
LOST3 = {"missing": [0, 1, 2]}
UNALIGNED = {"stripe_stride": NFRAGS * BS + 8}
ODD = {"blocksize": BS - 1}


def rs_code_text(entry):
    return "%s needs k + m <= 32 (k=30 m=4)" % ("check" if entry == "ecamd_rs_check" else "locate")


def code_fault(entry):
    """A code the entry point refuses, and the text it refuses it with."""
    if entry in RS_ENTRIES:
        return BIG, rs_code_text(entry)
    if entry in XOR_FULL:
        return {"hd": 5}, T_XOR_CODE
    if entry in XOR_DEG:
        return {"hd": 5}, T_DEG_CODE % 5
    if entry == "ecamd_rs_decode_masks":
        return {"k": 4, "m": 9}, "decode_masks needs k + m <= 32 and m <= 8 (k=4 m=9)"
    return {"hd": 5}, "(3,3,5) is not a flat_xor_hd code"


def cases():
    out = []

    def add(name, entry, over, text):
        out.append(pytest.param(entry, over, text, id="%s-%s" % (entry[6:], name)))

    for e in ENTRY:
        masks = e in MASKS
        layout = T_MASKS_LAYOUT if masks else T_LAYOUT
        over, text = code_fault(e)
        # ---- single faults ----
        add("code", e, over, text)
        add("null_base", e, {"base": None}, layout)
        add("null_lost" if masks else "null_status", e, {"lost" if masks else "status": None}, layout)
        add("negative_stripes", e, {"nstripes": -1}, layout)
        add("no_blocksize", e, {"blocksize": 0}, layout)
        add("short_stride", e, {"frag_stride": BS - 16}, layout)
        add("unaligned_base", e, {"base": "+8"}, T_ALIGN)
        add("unaligned_stripe_stride", e, UNALIGNED, T_ALIGN)
        add("unaligned_frag_stride", e, {"frag_stride": BS + 8}, T_ALIGN)
        if e in LOCATES:
            add("null_suspects", e, {"suspects": None}, "null suspects")
            add("odd_blocksize", e, ODD, T_ODD)
        if e in RS_MISSING:
            add("too_many_missing", e, LOST3, T_MISSING)
        if e in XOR_DEG:
            add("repeated_missing", e, {"missing": [1, 1]}, T_DEG_CODE % 3)
            add("missing_out_of_range", e, {"missing": [6]}, T_DEG_CODE % 3)
        # ---- double faults: which message wins ----
        add("code+null_base", e, dict(over, base=None), text)
        if e in RS_MISSING:
            add("null_base+too_many_missing", e, dict(LOST3, base=None), T_LAYOUT)
        if e in LOCATES:
            add("unaligned+odd_blocksize", e, dict(UNALIGNED, **ODD), T_ALIGN)
            add("null_suspects+odd_blocksize", e, dict(ODD, suspects=None), "null suspects")
        if e in XOR_DEG:
            add("repeated_missing+null_base", e, {"missing": [1, 1], "base": None}, T_DEG_CODE % 3)
            add("repeated_missing+unaligned", e, dict(UNALIGNED, missing=[1, 1]), T_DEG_CODE % 3)
    add("null_pairs", "ecamd_rs_locate_pairs", {"pairs": None}, "null pairs")
    add("null_pairs", "ecamd_rs_scrub_pairs", {"k": 10, "m": 4, "pairs": None}, "null pairs")
    add("null_pairs+too_many_missing", "ecamd_rs_locate_pairs", dict(LOST3, pairs=None), "null pairs")
    add("null_pairs+odd_blocksize", "ecamd_rs_locate_pairs", dict(ODD, pairs=None), T_ODD)
    add("m1", "ecamd_rs_scrub", {"m": 1}, "scrub needs m >= 2 to tell fragments apart (m=1)")
    add("m1+null_base", "ecamd_rs_scrub", {"m": 1, "base": None}, "scrub needs m >= 2 to tell fragments apart (m=1)")
    add("m2", "ecamd_rs_scrub_pairs", {"m": 2}, "a pair repair needs m >= 4 (m=2)")
    add("m2+null_base", "ecamd_rs_scrub_pairs", {"m": 2, "base": None}, "a pair repair needs m >= 4 (m=2)")
    add("m9+null_lost", "ecamd_rs_decode_masks", {"k": 4, "m": 9, "lost": None},
        "decode_masks needs k + m <= 32 and m <= 8 (k=4 m=9)")
    add("odd_blocksize", "ecamd_rs_decode_masks", ODD, "decode_masks needs an even blocksize (63)")
    add("unaligned+odd_blocksize", "ecamd_rs_decode_masks", dict(UNALIGNED, **ODD), T_ALIGN)
    add("null_lost+odd_blocksize", "ecamd_rs_decode_masks", dict(ODD, lost=None), T_MASKS_LAYOUT)
    return out


@pytest.mark.parametrize("entry,over,text", cases())
def test_refusal(ctx, entry, over, text):
    over = dict(over)
    if over.get("base") == "+8":
        over["base"] = ctx.frags.ptr + 8
    rc, host = ctx.call(entry, over)
    got = _lib.dev().ecamd_last_error().decode()
    print(entry, over, rc, repr(got))
    assert rc == EINVAL
    assert got == text
    assert all(v == (CANARY if name in ("checked", "covered") else ICANARY) for name, v in host.items()), host
    ctx.untouched()


PREBUILD = [
    ("null_arch", (4, 2, None, None, b"/nonexistent"), "null arch / dir"),
    ("null_dir", (4, 2, None, b"gfx950", None), "null arch / dir"),
    ("code", (30, 4, None, b"gfx950", b"/nonexistent"), "%s needs k + m <= 32 (k=30 m=4)"),
    ("too_many_missing", (4, 2, [0, 1, 2], b"gfx950", b"/nonexistent"), T_MISSING),
    ("code+null_dir", (30, 4, None, b"gfx950", None), "null arch / dir"),
    ("code+too_many_missing", (30, 4, [0, 1, 2], b"gfx950", b"/nonexistent"), "%s needs k + m <= 32 (k=30 m=4)"),
]


@pytest.mark.parametrize("what", ["check", "locate"])
@pytest.mark.parametrize("name,argv,text", PREBUILD, ids=[p[0] for p in PREBUILD])
def test_prebuild_refusal(what, name, argv, text):
    k, m, missing, arch, path = argv
    missing = _lib.ints(missing + [-1]) if missing is not None else None
    rc = getattr(_lib.dev(), "ecamd_%s_prebuild" % what)(k, m, missing, arch, path)
    got = _lib.dev().ecamd_last_error().decode()
    print(what, name, rc, repr(got))
    assert rc == EINVAL
    assert got == (text % what if "%s" in text else text)


STATUS_MASKS = [
    ("no_fragments", {"nfrag": 0}, 0), ("too_many_fragments", {"nfrag": 33}, 33), ("null_status", {"status": None}, 6),
    ("null_masks", {"result": None}, 6), ("negative_stripes", {"nstripes": -1}, 6),
    ("too_many_fragments+null_status", {"nfrag": 33, "status": None}, 33),
]


@pytest.mark.parametrize("name,over,nfrag", STATUS_MASKS, ids=[p[0] for p in STATUS_MASKS])
def test_frame_status_masks_refusal(ctx, name, over, nfrag):
    v = {"nfrag": 6, "status": ctx.frags.ptr, "bits": 1, "nstripes": S, "result": ctx.words.ptr + 4 * WORDS["result"]}
    v.update(over)
    rc = _lib.dev().ecamd_frame_status_masks(v["nfrag"], v["status"], v["bits"], v["nstripes"], v["result"], None)
    got = _lib.dev().ecamd_last_error().decode()
    print(name, rc, repr(got))
    assert rc == EINVAL
    assert got == "bad status_masks arguments (nfrag=%d)" % nfrag
    ctx.untouched()


def xor_covered(k, m, hd, missing):
    rows, sig, cov = (C.c_uint * 32)(), (C.c_uint * 32)(), C.c_uint(0)
    assert _lib.host().ecamd_xor_check_plan_degraded(k, m, hd, _lib.ints(list(missing) + [-1]), rows, sig, C.byref(cov)) >= 0
    return cov.value


EMPTY = [(e, {}) for e in ENTRY] + [(e, {"missing": [1]}) for e in RS_MISSING] + \
        [(e, {"k": 10, "m": 4}) for e in ("ecamd_rs_locate_pairs", "ecamd_rs_correct", "ecamd_rs_scrub_pairs")] + \
        [(e, {"missing": [0, 1, 3]}) for e in XOR_DEG]  # the last: no surviving row


@pytest.mark.parametrize("entry,over", EMPTY, ids=["%s-%s" % (e[6:], "_".join("%s%s" % kv for kv in o.items()) or "plain")
                                                   for e, o in EMPTY])
def test_empty_batch(ctx, entry, over):
    d = _lib.dev()
    before = [getattr(d, c)() for c in COUNTERS]
    rc, host = ctx.call(entry, dict(over, nstripes=0))
    assert rc == 0, d.ecamd_last_error().decode()
    assert [getattr(d, c)() for c in COUNTERS] == before, "an empty batch launched something"
    D.synchronize()
    ctx.untouched()
    k, m = over.get("k", 4), over.get("m", 2)
    missing = over.get("missing", [])
    if "checked" in host:  # every available fragment beyond the first k available ones
        avail = [f for f in range(k + m) if f not in missing]
        assert host["checked"] == sum(1 << f for f in avail[k:])
    if "covered" in host:
        assert host["covered"] == xor_covered(3, 3, 3, over.get("missing", [1]))
    assert all(host[n] == 0 for n in N4 if n in host), host
