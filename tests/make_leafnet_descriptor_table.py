"""Records what the leaf-net entries answer for a grid of descriptors - sizes, refusal codes and texts - so that a change of the
host side behind azmi_net_* can be replayed against the recording (tests/test_leafnet_descriptor_table.py):

    AZMI_LIB=<libazmi.so of the commit to record> python tests/make_leafnet_descriptor_table.py

writes tests/golden/leafnet_descriptor_table.json.  No device is needed and none may be present when recording: an accepted
descriptor is then recorded as AZMI_ERR_NO_DEVICE with the "no HIP device" text, the first thing the library says behind its
validation.

The grid (`grid()`, shared with the test): one accepted descriptor per family and tier (BASES), and around each of them every word
set, one at a time, to the values just inside and just outside each bound the library names (WORDS), the cross-cases its resolver
decides, the blob one byte off, and the entries' null checks.  Non-negative words only.  Per row: azmi_net_blob_bytes,
azmi_net_blob_bytes2, and azmi_net_create / azmi_net_create2 on a zero blob of the size the entry's own blob_bytes reported
(16 bytes where that is 0 or beyond BLOB_CAP) with the full azmi_net_last_error text.
"""
import ctypes as C
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "golden", "leafnet_descriptor_table.json")
BLOB_CAP = 8 << 20      # a size the library reports without validating can be anything: no blob beyond this
AZMI_OK, AZMI_ERR_INVALID, AZMI_ERR_NO_DEVICE = 0, -1, -2
NO_DEVICE_TEXT = "no HIP device: libazmi has no CPU path"

FIRST = ("in_channels", "height", "width", "channels", "depth", "kernel_size", "head_channels", "v_hidden", "num_moves", "num_players",
         "v_head_convs", "pi_head_convs", "v_fc_layers", "policy_channels", "precision", "pi_hidden")
SECOND = ("dense_net", "trunk_norm", "trunk_act", "pi_fc_layers")


def _d(**kw):
    d = dict.fromkeys(FIRST + SECOND, 0)
    d.update(kernel_size=3, num_players=2, v_fc_layers=1)
    d.update(kw)
    return d


def _resnet_c4(**kw):
    return _d(in_channels=4, height=6, width=7, channels=64, depth=1, head_channels=32, v_hidden=64, num_moves=7, **kw)


def _resnet_sp(b, glob=0, **kw):
    return _d(in_channels=6, height=b, width=b, channels=64, depth=1, head_channels=64, v_hidden=128, num_moves=4 * b * b + glob,
              v_head_convs=1, pi_head_convs=1, policy_channels=4, pi_hidden=64 if glob else 0, **kw)


def _dense_c4(**kw):
    return _d(in_channels=4, height=6, width=7, channels=8, depth=2, head_channels=32, v_hidden=32, num_moves=7, dense_net=1, **kw)


def _dense_sp(b, glob=0, **kw):
    return _d(in_channels=6, height=b, width=b, channels=8, depth=2, head_channels=32, v_hidden=32, num_moves=4 * b * b + glob,
              policy_channels=4, pi_hidden=32 if glob else 0, dense_net=1, **kw)


# one accepted descriptor per family and tier (depth 1 or 2: no blob above about a megabyte)
BASES = {
    "c4_bf16": _resnet_c4(), "c4_bf16x3": _resnet_c4(precision=2),
    "sp7_bf16": _resnet_sp(7), "sp11_bf16": _resnet_sp(11), "sp13_bf16": _resnet_sp(13, glob=19),
    "sp7_bf16x3": _resnet_sp(7, precision=2), "sp11_bf16x3": _resnet_sp(11, precision=2), "sp13_bf16x3": _resnet_sp(13, glob=19, precision=2),
    "dense_k3": _dense_c4(), "dense_k5": _dense_c4(kernel_size=5), "dense_layer": _dense_c4(trunk_norm=1),
    "dsp7": _dense_sp(7), "dsp11": _dense_sp(11, glob=19), "dsp13": _dense_sp(13, glob=19, kernel_size=5),
    "f32_resnet": _resnet_c4(precision=1), "f32_dense": _dense_c4(precision=1),
    "f32_resnet_layer": _resnet_c4(precision=1, trunk_norm=1), "f32_dense_layer": _dense_c4(precision=1, trunk_norm=1),
    "f32_resnet_crelu": _resnet_c4(precision=1, trunk_act=1), "f32_dense_crelu": _dense_c4(precision=1, trunk_act=1),
    "f32_resnet_pifc": _resnet_c4(precision=1, pi_fc_layers=1, pi_hidden=32), "f32_dense_pifc": _dense_c4(precision=1, pi_fc_layers=2, pi_hidden=32),
}
# the bases the first entry accepts too: the families behind dense_net and the variant words exist on the second descriptor alone
ACCEPTED_BY_CREATE = {n for n, d in BASES.items() if not any(d[w] for w in SECOND)}

# both sides of every bound the library names for a word, whichever family names it
WORDS = {
    "in_channels": (0, 1, 4, 5, 8, 9, 64, 65, 112, 113),
    "channels": (0, 1, 16, 17, 63, 64, 65),
    "depth": (0, 1, 2, 6, 7),
    "kernel_size": (0, 1, 2, 3, 4, 5, 6, 7, 9),
    "head_channels": (0, 31, 32, 33, 63, 64, 65),
    "v_hidden": (0, 15, 16, 17, 32, 127, 128, 129, 256, 257, 272, 384, 512, 513, 640),
    "num_players": (0, 1, 3, 4, 15, 16),
    "v_head_convs": (0, 1, 2), "pi_head_convs": (0, 1, 2), "v_fc_layers": (0, 1, 2, 3),
    "policy_channels": (0, 1, 32, 33),
    "precision": (0, 1, 2, 3),
    "pi_hidden": (0, 1, 15, 16, 17, 63, 64, 65, 128, 256, 257, 272, 1024, 1025, 1088),
    "dense_net": (0, 1, 2), "trunk_norm": (0, 1, 2), "trunk_act": (0, 1, 2), "pi_fc_layers": (0, 1, 2),
}
BOARDS = ((6, 7), (7, 6), (7, 7), (7, 11), (9, 9), (11, 11), (13, 13), (15, 15))


def _moves(d):
    """num_moves around the flat head's bounds and around the spatial block of `d` (0..32 global actions behind it)"""
    block = d["policy_channels"] * d["height"] * d["width"]
    return sorted({0, 1, 16, 17} | ({block - 1, block, block + 1, block + 32, block + 33} if block else set()))


def grid():
    """[(row name, words or None, blob delta)]: words = the 20 named words plus `reserved` (four of them); None = a null descriptor"""
    rows = [("null", None, 0)]
    for name, base in BASES.items():
        def row(tag, delta=0, **kw):
            d = dict(base, reserved=(0, 0, 0, 0))
            d.update(kw)
            rows.append(("%s/%s" % (name, tag), d, delta))
        row("base")
        row("blob+1", 1)
        row("blob-1", -1)
        for word, values in WORDS.items():
            for v in values:
                if v != base[word]:
                    row("%s=%d" % (word, v), **{word: v})
        for h, w in BOARDS:
            if (h, w) != (base["height"], base["width"]):
                # (a spatial head keeps its block: the board is the word under test, not num_moves)
                glob = base["num_moves"] - base["policy_channels"] * base["height"] * base["width"]
                row("board=%dx%d" % (h, w), height=h, width=w, num_moves=base["policy_channels"] * h * w + glob if base["policy_channels"] else base["num_moves"])
        for m in _moves(base):
            if m != base["num_moves"]:
                row("num_moves=%d" % m, num_moves=m)
        for i in range(4):
            row("reserved[%d]=1" % i, reserved=tuple(int(j == i) for j in range(4)))
        # what the resolver decides between the families and tiers
        row("spatial_head_on_6x7", height=6, width=7, policy_channels=4, num_moves=4 * 42)
        row("pi_fc_stack_without_width", pi_fc_layers=1, pi_hidden=0)
        row("pi_fc_stack_on_spatial_head", pi_fc_layers=1, policy_channels=max(base["policy_channels"], 1), pi_hidden=32)
        for p in (0, 1, 2):
            row("crelu_p%d" % p, trunk_act=1, precision=p)
            row("layer_p%d" % p, trunk_norm=1, precision=p)
            row("dense_p%d" % p, dense_net=1, precision=p)
            row("dense_layer_p%d" % p, dense_net=1, trunk_norm=1, precision=p)
            row("dense_net=2_p%d" % p, dense_net=2, precision=p)
            row("dense_net=2_layer_p%d" % p, dense_net=2, trunk_norm=1, precision=p)
    assert len({r[0] for r in rows}) == len(rows)
    return rows


class Desc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in FIRST]


class Desc2(C.Structure):
    _fields_ = [("base", Desc)] + [(n, C.c_int32) for n in SECOND] + [("reserved", C.c_int32 * 4)]


def load(path):
    lib = C.CDLL(path)
    for fn, desc in (("azmi_net_blob_bytes", Desc), ("azmi_net_blob_bytes2", Desc2)):
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = C.c_size_t, [C.POINTER(desc)]
    for fn, desc in (("azmi_net_create", Desc), ("azmi_net_create2", Desc2)):
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = C.c_int, [C.POINTER(desc), C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
    lib.azmi_net_destroy.restype, lib.azmi_net_destroy.argtypes = None, [C.c_void_p]
    lib.azmi_net_last_error.restype = C.c_char_p
    return lib


def answers(lib, words, delta):
    """[blob_bytes, blob_bytes2, rc of create, its text, rc of create2, its text] of one row; a net that was created is destroyed"""
    if words is None:
        d1 = d2 = None
    else:
        d1 = Desc(*[words[n] for n in FIRST])
        d2 = Desc2(d1, *[words[n] for n in SECOND], (C.c_int32 * 4)(*words["reserved"]))
    out = [int(lib.azmi_net_blob_bytes(d1)), int(lib.azmi_net_blob_bytes2(d2))]
    for create, d, size in ((lib.azmi_net_create, d1, out[0]), (lib.azmi_net_create2, d2, out[1])):
        n = max((size if 0 < size <= BLOB_CAP else 16) + delta, 1)
        blob = C.create_string_buffer(n)
        h = C.c_void_p()
        rc = create(d, blob, n, 0, C.byref(h))
        out += [rc, "" if rc == AZMI_OK else lib.azmi_net_last_error().decode()]
        if rc == AZMI_OK:
            lib.azmi_net_destroy(h)
    return out


# Every text the parent's csrc/leafnet.hip can refuse a DESCRIPTOR with (a `%` conversion as a pattern).  Its other texts need a
# device or a live net (no HIP device, hipSetDevice, hipMalloc, upload, LDS reservation, launches, the trunk read-out on a tile),
# and two cannot be reached through its own earlier checks: "spatial head: logits do not fit the tile's LDS" (at most 32 policy
# channels and 32 global actions on the three boards stay under the ring) and "v_hidden / pi_hidden above 1024"
REFUSALS = [
    r"null argument", r"precision must be 0 \(bf16 MFMA\), 1 \(fp32\) or 2 \(bf16x3: split bf16 MFMA\)",
    r"spatial leaf net kernel covers 64 trunk / 64 head channels, 3x3 convs, one extra conv per head", r"spatial leaf net kernel: board \d+x\d+ not instantiated",
    r"spatial head: policy channels <= 32, 0\.\.32 global actions", r"spatial head with global actions: pi_hidden must be a multiple of 64 in \[64, 1024\]",
    r"spatial leaf net kernel: \d+ input planes not supported", r"spatial leaf net kernel: 1\.\.6 residual blocks", r"value head sizes out of range",
    r"weight blob is \d+ bytes, expected \d+",
    r"leaf net kernel covers 64 trunk channels, 32 head channels, 3x3 convs", r"leaf net kernel: board \d+x\d+ not instantiated",
    r"leaf net kernel: \d+ input planes not instantiated \(Connect4 has 4\)", r"leaf net kernel: 1\.\.6 residual blocks",
    r"head sizes out of range \(v_hidden: a multiple of 16, at most 256\)",
    r"azmi_net_desc2: reserved words must be zero", r"azmi_net_desc2: dense_net must be 0 or 1",
    r"azmi_net_desc2: trunk_norm must be 0 \(batch\) or 1 \(layer\)", r"azmi_net_desc2: trunk_act must be 0 \(relu\) or 1 \(crelu\)",
    r"azmi_net_desc2: pi_fc_layers > 0 is the flat policy head's FC stack \(policy_channels must be 0\)",
    r"azmi_net_desc2: pi_fc_layers > 0 needs pi_hidden \(the stack's width\)",
    r"the matrix-core tiles cover trunk_act='relu' and pi_fc_layers=0, .*", r"dense spatial leaf net kernel: trunk_norm='batch' only .*",
    r"dense leaf net: no bf16x3 tier; .*", r"precision must be 0 \(bf16 MFMA\) or 1 \(fp32\) for a dense net",
] + [r"dense leaf net kernel" + t + r"; use precision='fp32' for other shapes" for t in (
    r" covers the 6x7 board with the flat policy head", r": kernel_size 3 or 5", r": growth rate \(channels\) 1\.\.16", r": at least one block and one input plane",
    r": in_channels \+ channels \* depth <= 128", r": 32 head channels, no extra head convolutions, one value FC layer", r": head sizes out of range \(.*\)")
] + [r"dense spatial leaf net kernel" + t + r"; use precision='fp32' for other shapes" for t in (
    r" covers 7x7, 11x11 and 13x13 boards", r": kernel_size 3 or 5", r": growth rate \(channels\) 1\.\.16", r": at least one block and one input plane",
    r": in_channels \+ channels \* depth <= 128", r": 32 head channels, no extra head convolutions, one value FC layer",
    r": policy channels 1\.\.32, 0\.\.32 global actions", r": pi_hidden must be a multiple of 16 in 16\.\.256 with global actions", r": head sizes out of range \(.*\)")]
# (the one word no non-negative value takes out of its range - "azmi_net_desc2: pi_fc_layers must be >= 0" - is not in the table)


def accepted(rc, text):
    return rc == AZMI_ERR_NO_DEVICE and text == NO_DEVICE_TEXT


def main():
    lib = load(os.environ["AZMI_LIB"])
    rows = {name: answers(lib, words, delta) for name, words, delta in grid()}
    texts = [t for r in rows.values() for t in (r[3], r[5])]
    for pattern in REFUSALS:
        assert any(re.fullmatch(pattern, t) for t in texts), "no row is refused with: " + pattern
    for name in BASES:
        r = rows[name + "/base"]
        assert r[1] > 0 and accepted(r[4], r[5]), (name, r)
        assert name not in ACCEPTED_BY_CREATE or (r[0] > 0 and accepted(r[2], r[3])), (name, r)
    # the texts once, the rows by index: [blob_bytes, blob_bytes2, rc, text, rc2, text2]
    index = sorted(set(texts))
    at = {t: i for i, t in enumerate(index)}
    with open(TABLE, "w") as f:
        json.dump({"texts": index, "rows": {n: [r[0], r[1], r[2], at[r[3]], r[4], at[r[5]]] for n, r in rows.items()}}, f, separators=(",", ":"))
        f.write("\n")
    print("%d rows, %d texts, %d bytes -> %s" % (len(rows), len(index), os.path.getsize(TABLE), TABLE))


if __name__ == "__main__":
    sys.exit(main())
