"""The resize family -- vacv_resize, vacv_resize_normalize and the fused
statistics calls (csrc/k_resize.hip, k_resize_direct.hip, k_resize_strip.hip,
k_cubic_direct.hip, k_lanczos.hip, k_area.hip and the NEAREST / AREA kernels
of k_pixel.hip) -- at the misaligned, pitched and tail placements that select
their kernels, load widths and store widths, and across the eviction of the
device-side caches they keep.

The host selectors and many in-kernel branches of these kernels depend on the
low bits of the base address and of the row, plane and image pitches.  As in
test_gpu_plumbing every source and destination here is a view placed inside a
larger device buffer, so a case controls those bits exactly: the padding of a
u8 source holds SENTINEL bytes and that of an fp32 source the float 1e30 (a
stray read of it cannot vanish in rounding), and a destination's padding must
still hold SENTINEL afterwards.  SRC_PLACEMENTS and DST_PLACEMENTS name the
placements; PATHS names every (interpolation, source type, output kind,
tuning knobs) combination; CASES is a deterministic selection of (path,
placements, channels, geometry), not the cross product, and
test_case_list_covers_every_pair (CPU) asserts what it must contain.

The reference is the oracle's C restatement of each operator on a dense copy
of each image, as test_gpu_parity uses it.  Every comparison is bit for bit,
with the one exception of the project's parity bar: the sign of an exact zero
in an fp32 cubic result (a zero-weight tap row is skipped), compared by value
as test_gpu_parity.assert_same does.  No tolerances, except the project's own
1e-6 relative bound of the fused cubic sums (test_resize_channel_sums).

All GPU tests carry the gpu mark one by one because the coverage test and the
checker's self-test must run without a device.
"""
from __future__ import annotations

import collections
import zlib

import numpy as np
import pytest

from test_gpu_colour import place_planes
from test_gpu_parity import assert_same
from test_gpu_plumbing import (SENTINEL, assert_bits, assert_rim_intact, assert_untouched, blank, host, place,
                               unsupported)

gpu = pytest.mark.gpu
NHWC, NCHW = 1, 0  # include/vacv_hip.h; asserted against the package in the ops fixture
INTERP = {"NEAREST": 0, "LINEAR": 1, "CUBIC": 2, "AREA": 3, "LANCZOS4": 4}
MEAN = np.array([103.94, 116.78, 123.68, 99.5], np.float32)
STD = np.array([57.375, 57.12, 58.395, 61.25], np.float32)
LOUD = np.float32(1e30)  # the padding of fp32 sources: finite (a zero weight still gives 0), loud under any other


@pytest.fixture(scope="module")
def ops(hip_device):
    import vacv_amd as V
    from vacv_amd import ops
    assert (V.NHWC, V.NCHW) == (NHWC, NCHW)
    assert {k: getattr(V, "INTER_" + k) for k in INTERP} == INTERP
    return ops


@pytest.fixture(scope="module")
def dev(hip_device):
    return hip_device


# ---------------------------------------------------------------------------
# placements

# off: the base's offset in elements (1 byte for u8, 4 for fp32), or in bytes
# where off_bytes is given; row: "dense", "p16" (padded up to a multiple of 16
# bytes, by at least one element) or "odd" (+5 elements u8, +1 fp32); img: the
# pad after every image in elements, "mis" = 16 / es - 1 (image 1 starts 1
# element short of a 16-byte boundary); plane "mis": the pad after every NCHW
# plane that makes plane 1 start 1 element past a 16-byte boundary.
SRC_PLACEMENTS = {
    "dense": dict(off=0, row="dense", img=0),       # the baseline
    "off1": dict(off=1, row="dense", img=0),        # every `bits & 15` and `& 3` fallback
    "off4": dict(off_bytes=4, row="dense", img=0),  # u8 only: dword-aligned, not 16: area lane / colsum(4)
    "p16": dict(off=0, row="p16", img=0),           # strip, unit, row-staged NEAREST with a real pad
    "off_p16": dict(off=1, row="p16", img=0),       # the strip kernel with a misaligned base
    "odd": dict(off=0, row="odd", img=3),           # rows at every alignment; image 1 misaligned
    "img_mis": dict(off=0, row="p16", img="mis"),   # `bits` through img_pitch only
    "planes": dict(off=0, row="dense", img=3, plane="mis"),  # NCHW only: `bits` through plane_pitch
}
DST_PLACEMENTS = {k: v for k, v in SRC_PLACEMENTS.items() if k != "off4"}
U8_ONLY = {"off4"}
NCHW_ONLY = {"planes"}
IMG_PITCH_MATTERS = {"odd", "img_mis", "planes"}  # batches of 3 there, of 2 elsewhere


def pads(spec, layout, shape, es):
    """(offset in bytes, row pad, plane pad, batch pad) of a placement for an image batch of `shape`."""
    if layout == NHWC:
        _, h, w, c = shape
        re = w * c
    else:
        _, _, h, re = shape
    q = 16 // es
    row = {"dense": 0, "p16": q - re % q, "odd": 5 if es == 1 else 1}[spec["row"]]
    img = q - 1 if spec["img"] == "mis" else spec["img"]
    plane = ((1 - h * (re + row)) % q or q) if layout == NCHW and spec.get("plane") == "mis" else 0
    return spec.get("off_bytes", spec.get("off", 0) * es), row, plane, img


def strides_of(shape, layout, row_pad, plane_pad, batch_pad):
    if layout == NHWC:
        n, h, w, c = shape
        rp = w * c + row_pad
        img = h * rp + batch_pad
        return (img, rp, c, 1), img
    n, c, h, w = shape
    rp = w + row_pad
    pl = h * rp + plane_pad
    img = c * pl + batch_pad
    return (img, pl, rp, 1), img


def place_f32(a, dev, layout, off, row_pad, plane_pad, batch_pad):
    """`place` / `place_planes` for an fp32 SOURCE: the same layout, every byte
    outside the view holding the float 1e30 (0xA5A5A5A5 as a float is about
    -2.9e-16: a stray read of it vanishes in rounding)."""
    import torch
    a = np.ascontiguousarray(a, np.float32)
    assert off % 4 == 0
    strides, img = strides_of(a.shape, layout, row_pad, plane_pad, batch_pad)
    n = a.shape[0]
    flat = np.full(off // 4 + n * img + 8, LOUD, np.float32)
    np.lib.stride_tricks.as_strided(flat[off // 4:], a.shape, [4 * s for s in strides])[...] = a
    buffer = torch.from_numpy(flat).to(dev)
    return buffer, buffer[off // 4:off // 4 + n * img].as_strided(a.shape, strides)


def place_as(a, dev, layout, name, table, source):
    """(buffer, view) of `a` placed as table[name]; a source's fp32 padding is loud."""
    a = np.ascontiguousarray(a)
    off, rpad, ppad, bpad = pads(table[name], layout, a.shape, a.itemsize)
    if source and a.dtype == np.float32:
        return place_f32(a, dev, layout, off, rpad, ppad, bpad)
    if layout == NHWC:
        return place(a, dev, NHWC, off=off, row_pad=rpad, batch_pad=bpad)
    return place_planes(a, dev, off=off, row_pad=rpad, plane_pad=ppad, batch_pad=bpad)


def check_placed(dbuf, dview, want, what, by_value=False):
    """The checker: the view equals `want` -- bit for bit, or by value where
    the parity bar allows an exact zero's sign to differ -- and every byte of
    the buffer outside the view still holds SENTINEL."""
    got = host(dview)
    if by_value:
        assert_same(np.ascontiguousarray(got), np.ascontiguousarray(want), what)
    else:
        assert_bits(got, want, what)
    assert_rim_intact(dbuf, dview, what)


# ---------------------------------------------------------------------------
# paths: (interpolation, source type, output kind, tuning knobs)

Path = collections.namedtuple("Path", "interp dtype out knobs geoms")


def _paths():
    P = {}
    for out in ("same", "norm"):
        for name, knobs in [("gather", dict(RESIZE_DIRECT=2)), ("strip1", dict(RESIZE_DIRECT=0, RESIZE_STRIP=1)),
                            ("strip2", dict(RESIZE_DIRECT=0, RESIZE_STRIP=2)),
                            ("staged", dict(RESIZE_DIRECT=0, RESIZE_STRIP=0)), ("default", {})]:
            P[f"lin_u8_{name}_{out}"] = Path("LINEAR", "u8", out, knobs, "gen")
        P[f"lin_f32_{out}"] = Path("LINEAR", "f32", out, {}, "gen")
        for k in (1, 2, 0):
            P[f"cubic_u8_cd{k}_{out}"] = Path("CUBIC", "u8", out, dict(CUBIC_DIRECT=k), "gen")
        P[f"cubic_f32_{out}"] = Path("CUBIC", "f32", out, {}, "gen")
        for dt in ("u8", "f32"):
            for name, knobs in [("default", {}), ("row", dict(NEAREST_KERNEL=1)), ("pixel", dict(NEAREST_KERNEL=0))]:
                P[f"nearest_{dt}_{name}_{out}"] = Path("NEAREST", dt, out, knobs, "gen")
        for name, knobs in [("default", {}), ("k3", dict(AREA_KERNEL=3)), ("k2", dict(AREA_KERNEL=2)),
                            ("k1", dict(AREA_KERNEL=1))]:
            P[f"area_u8_{name}_{out}"] = Path("AREA", "u8", out, knobs, "area")
        P[f"area_f32_{out}"] = Path("AREA", "f32", out, {}, "area")
        for dt in ("u8", "f32"):
            P[f"areaany_{dt}_{out}"] = Path("AREA", dt, out, {}, "areaany")
        for k in (0, 2, 1):
            P[f"lanczos_u8_k{k}_{out}"] = Path("LANCZOS4", "u8", out, dict(LANCZOS_KERNEL=k), "lanczos")
        P[f"lanczos_f32_{out}"] = Path("LANCZOS4", "f32", out, {}, "lanczos")
    P["lanczos_narrow_u8_same"] = Path("LANCZOS4", "u8", "same", {}, "narrow")
    P["lanczos_narrow_u8_norm"] = Path("LANCZOS4", "u8", "norm", {}, "narrow")
    P["lanczos_narrow_f32_same"] = Path("LANCZOS4", "f32", "same", {}, "narrow")
    return P


PATHS = _paths()

# (source rows, source columns, output rows, output columns).  Output widths 5
# (a partial lane quad), 64 (one whole strip), 67 (a strip + 3) and 131 (two
# strips + 3, byte-store tails); output heights 1, 9 and 37 leave a partial
# last row group or band.  With 1 to 4 channels the output rows are a multiple
# of 16 bytes (width 64) and not (5, 67, 131: e.g. c = 3 gives 192 against 201
# bytes, and as fp32 768 against 804): the kernels' `chunked` store conditions.
GEN = [(63, 128, 9, 64),    # rows 7:1 (one weighted source row each: the gather kernel's ONE_ROW instance), columns 2:1
       (54, 96, 36, 64),    # 3:2 exactly
       (54, 100, 37, 67),   # about 3:2, a strip + 3
       # an up-scale: the last output rows and columns tap the last source row and column of the LAST image, so
       # the final 16-byte or 8-byte load of the batch overhangs the plane and the view (as in every up-scale)
       (40, 50, 57, 131),
       (41, 67, 9, 67),     # equal width, another height
       (40, 51, 1, 5),      # one row, a partial quad
       (45, 60, 37, 131)]   # down in y, up in x
# Lanczos also at 9.4:1 in x: a strip's windows span about 590 * cc bytes, so
# lanczos_run_loads gives run_ni 1 (cc = 1, NCHW planes too), 2 (cc = 3) and 0 (cc = 4)
WIDE = (24, 600, 9, 64)
NARROW = [(40, 6, 9, 5), (20, 5, 37, 17), (41, 7, 9, 67)]  # narrower than the 8-pixel row window
# INTER_AREA with integer blocks (ax, ay): 2 x 2 (half up for c = 1, 3, 4, half
# to even for c = 2: a quarter of random blocks are ties), 3 x 3, 4 x 2, 3 x 2.
# Which kernel a case runs depends on the source's alignment as well
# (area_kernel below restates launch_resize_area's selector).  AREA rotates
# through every path at widths whose dense rows are mostly odd; AREA_X holds
# the geometries of AREA_KERNEL_CASES, whose dense rows are multiples of 16
# (output width 64) or of 4 (68) bytes, so that the unit, lane and column-sum
# kernels are what runs at the dense, off4 and p16 placements.
AREA_BLOCKS = [(2, 2), (3, 3), (4, 2), (3, 2)]
AREA_OUTS = [(9, 64), (37, 33), (1, 5), (13, 67)]
AREA = [(AREA_OUTS[(i + i // 4) % 4][0] * AREA_BLOCKS[i % 4][1], AREA_OUTS[(i + i // 4) % 4][1] * AREA_BLOCKS[i % 4][0])
        + AREA_OUTS[(i + i // 4) % 4] for i in range(16)]
AREAANY = [(48, 80, 37, 67), (48, 80, 57, 131), (48, 80, 61, 64), (48, 80, 9, 100)]  # down, up, mixed, mixed
# (ax, ay, c): every area_unit_applies instance (AX 2 or 4 with 1-4 channels, AX 3 with one) and both
# area_lane_applies ones (AX 3 with 3 or 4 channels) with 3 and 2 block rows (the kernel's area_y == 3 branch)
AREA_INSTANCES = [(3, 3, 3), (3, 3, 4), (3, 2, 3), (3, 2, 4), (4, 2, 1), (4, 2, 2), (4, 2, 3), (4, 2, 4), (2, 2, 1),
                  (2, 2, 2), (2, 2, 3), (2, 2, 4), (3, 3, 1)]


def area_geom(ax, ay, ho, wo):
    return (ho * ay, wo * ax, ho, wo)


# widths 64 and 68; 272 = 256 + 16: a whole wave of the lane kernel's 4-pixel lanes (c = 3) and a partial one
AREA_X = sorted({area_geom(ax, ay, ho, wo) for ax, ay, _ in AREA_INSTANCES for ho in (9, 1, 5) for wo in (64, 68)}
                | {area_geom(3, ay, 2, 272) for ay in (3, 2)})
ROTATED = {"gen": GEN, "lanczos": GEN + [WIDE], "narrow": NARROW, "area": AREA, "areaany": AREAANY}
GEOMS = dict(ROTATED, area=AREA + AREA_X)
CHANS = [1, 2, 3, 4, "chw"]  # NHWC channel counts, and NCHW with 3 planes

Case = collections.namedtuple("Case", "path src dst chan geom mode")


def admitted(placements, path, chan=None):
    names = [s for s in placements if not (s in U8_ONLY and path.dtype != "u8")]
    if chan is not None:
        names = [s for s in names if (s in NCHW_ONLY) <= (chan == "chw")]
    return names


def _area_kernel_cases():
    """Every unit and lane instance under the default knob and AREA_KERNEL=3, at a 16-aligned source (dense,
    width 64), a 4-aligned one (dense, width 68), a base at 4 mod 16 (off4), a padded 16-multiple pitch (p16)
    and an image pitch that alone misaligns image 1 (img_mis)."""
    A = []
    for path in ("area_u8_default_same", "area_u8_k3_same", "area_u8_default_norm"):
        for i, (ax, ay, c) in enumerate(AREA_INSTANCES):
            for j, s in enumerate(("dense", "off4", "p16", "img_mis")):
                for wo in (64, 68) if path.endswith("same") else (64,):
                    d = ("dense", "p16", "off1", "odd")[(i + j) % 4]
                    A.append(Case(path, s, d, c, area_geom(ax, ay, (9, 1, 5)[(i + j) % 3], wo), 0))
        for ay in (3, 2):
            for s in ("dense", "off4", "p16"):
                A.append(Case(path, s, "dense", 3, area_geom(3, ay, 2, 272), 0))
    return A


AREA_KERNEL_CASES = _area_kernel_cases()


def _headline_cases():
    H = []
    # 1. strip kernel x a misaligned base with a 16-multiple pitch
    for sv in ("strip1", "strip2"):
        for i, c in enumerate((1, 3, 4)):
            for mode in (0, 1, 2):
                H.append(Case(f"lin_u8_{sv}_same", "off_p16", "dense", c, GEN[1 + (i + mode) % 3], mode))
        for mode in (0, 1, 2):
            H.append(Case(f"lin_u8_{sv}_norm", "off_p16", "dense", 3, GEN[1 + mode], mode))
    # 2. NEAREST / AREA selectors through the image pitch alone, and a base at 4 mod 16
    for p in ("nearest_u8_default_same", "nearest_u8_row_same", "nearest_f32_default_same", "nearest_f32_row_same"):
        H.append(Case(p, "img_mis", "dense", 3, GEN[2], 0))
    # a dense u8 / fp32 source with 16-multiple rows: the aligned baseline of the row-staged kernels
    for p in ("nearest_u8_default_same", "nearest_u8_row_same", "nearest_f32_default_same", "nearest_f32_row_same",
              "nearest_u8_default_norm", "nearest_u8_row_norm"):
        for c in (1, 3, 4):
            H.append(Case(p, "dense", "dense", c, GEN[0], 0))
    H += AREA_KERNEL_CASES
    # 3. cubic column kernel (16-aligned destination, 768-byte rows) or gather (the others)
    for d in ("dense", "p16", "off1", "img_mis"):
        H.append(Case("cubic_u8_cd1_same", "dense", d, 3, GEN[1], 0))
        H.append(Case("cubic_u8_cd1_norm", "dense", d, 3, GEN[1], 0))
    H.append(Case("cubic_u8_cd2_same", "dense", "p16", 3, GEN[2], 0))  # 804-byte rows: `chunked` false, pitched
    H.append(Case("cubic_u8_cd2_norm", "dense", "p16", 3, GEN[2], 0))
    # 4. bilinear gather x a pitched destination, rows of 192 / 768 bytes and of 201 / 804
    for p in ("lin_u8_gather_same", "lin_u8_gather_norm"):
        for g in (GEN[0], GEN[2]):
            for mode in (0, 1, 2):
                H.append(Case(p, "dense", "p16", 3, g, mode))
    # 5. Lanczos, all three knobs and fp32, x misaligned and pitched operands
    for p in ("lanczos_u8_k0_same", "lanczos_u8_k2_same", "lanczos_u8_k1_same", "lanczos_f32_same",
              "lanczos_u8_k0_norm", "lanczos_f32_norm"):
        for i, s in enumerate(("off1", "odd", "p16")):
            H.append(Case(p, s, "dense", 3, GEN[(2 + i) % 7], 0))
        for i, d in enumerate(("off1", "odd")):
            H.append(Case(p, "dense", d, 3, GEN[(3 + i) % 7], 0))
    for p in ("lanczos_u8_k0_same", "lanczos_u8_k2_same", "lanczos_u8_k1_same", "lanczos_u8_k0_norm"):
        for c in (1, 3, 4, "chw"):  # run_ni 1, 2, 0, 1; the run's 16 more bytes for a misaligned base
            H.append(Case(p, "off1", "off1", c, WIDE, 0))
    # 6. staged kernel x rows at every alignment and a misaligned base
    for p in ("lin_u8_staged_same", "lin_f32_same", "cubic_u8_cd0_same", "cubic_f32_same"):
        for i, s in enumerate(("odd", "off1")):
            H.append(Case(p, s, "dense", 3, GEN[(1 + 2 * i) % 7], i))
    return H


def _build_cases():
    """Per path: one case per admitted source placement, the destination
    placement, channel count and geometry rotating with it; then whatever
    destination or channel count the rotation missed; then the headline
    pairs.  Deterministic, and far smaller than the cross product."""
    dsts = list(DST_PLACEMENTS)
    cases = []
    for pi, (name, p) in enumerate(PATHS.items()):
        geoms = ROTATED[p.geoms]
        mine = []
        for k, s in enumerate(admitted(SRC_PLACEMENTS, p)):
            d = dsts[(k + pi) % len(dsts)]
            ch = "chw" if NCHW_ONLY & {s, d} else CHANS[(k + 2 * pi) % 5]
            mine.append(Case(name, s, d, ch, geoms[(k + 3 * pi) % len(geoms)], (k + pi) % 3))
        for j, d in enumerate(x for x in dsts if x not in {c.dst for c in mine}):
            mine.append(Case(name, "dense", d, "chw" if d in NCHW_ONLY else CHANS[(j + pi) % 5],
                             geoms[(j + pi) % len(geoms)], j % 3))
        for j, ch in enumerate(x for x in CHANS if x not in {c.chan for c in mine}):
            srcs = admitted(SRC_PLACEMENTS, p, ch)
            mine.append(Case(name, srcs[(j + pi) % len(srcs)], admitted(DST_PLACEMENTS, p, ch)[(j + 2 * pi) % 5], ch,
                             geoms[(j + 2 * pi) % len(geoms)], (j + 1) % 3))
        cases += mine
    for c in _headline_cases():
        if c not in cases:
            cases.append(c)
    return cases


CASES = _build_cases()


def batch_of(c):
    return 3 if IMG_PITCH_MATTERS & {c.src, c.dst} else 2


def src_pitches(c):
    """(base offset, row pitch, plane pitch, image pitch) in bytes of the
    case's source, as the descriptor carries them: the allocator's base is
    512-byte aligned, so these are the bits the host selectors OR together."""
    es = 1 if PATHS[c.path].dtype == "u8" else 4
    h, w = c.geom[:2]
    layout = NCHW if c.chan == "chw" else NHWC
    shape = (batch_of(c), 3, h, w) if layout == NCHW else (batch_of(c), h, w, c.chan)
    off, rpad, ppad, bpad = pads(SRC_PLACEMENTS[c.src], layout, shape, es)
    strides, img = strides_of(shape, layout, rpad, ppad, bpad)
    dense_row = (w if layout == NCHW else w * c.chan) * es
    row = strides[2 if layout == NCHW else 1] * es if h > 1 else dense_row  # a single row: the dense pitch
    return off, row, strides[1] * es if layout == NCHW else 0, img * es


def area_kernel(c):
    """launch_resize_area's choice (k_pixel.hip) for an integer-block AREA case:
    "unit", "lane", "colsum16", "colsum4" or "pixel"."""
    p = PATHS[c.path]
    if p.dtype != "u8":
        return "pixel"
    h, w, ho, wo = c.geom
    ax, cc = w // wo, 1 if c.chan == "chw" else c.chan
    off, row, plane, img = src_pitches(c)
    bits = off | row | plane | img
    knob = p.knobs.get("AREA_KERNEL", -1)
    unit = ax in (2, 4) or (ax == 3 and cc == 1)   # area_unit_applies
    lane = ax == 3 and cc in (3, 4)                # area_lane_applies
    if bits & 15 == 0 and knob <= 0 and unit:
        return "unit"
    if bits & 3 == 0 and knob <= 0 and lane:
        return "lane"
    vb = 16 if bits & 15 == 0 else 4 if bits & 3 == 0 else 0
    if vb and knob != 1:
        return "colsum4" if knob == 2 else f"colsum{vb}"
    return "pixel"


def nearest_kernel(c):
    """launch_resize_nearest's choice (k_pixel.hip): "wave", "row" or "pixel"."""
    p = PATHS[c.path]
    es = 1 if p.dtype == "u8" else 4
    h, w, ho, wo = c.geom
    cc = 1 if c.chan == "chw" else c.chan
    off, row, plane, img = src_pitches(c)
    aligned = (off | row | plane | img) & 15 == 0
    dense_samples = w / wo * cc * es <= 128.0
    knob = p.knobs.get("NEAREST_KERNEL", -1)
    if aligned and w * cc * es <= 16 * 1024 and dense_samples and knob not in (0, 1):
        return "wave"
    if aligned and w * cc * es <= 64 * 1024 and dense_samples and knob != 0:
        return "row"
    return "pixel"


def cases_of(prefix):
    return [c for c in CASES if c.path.startswith(prefix)]


def case_id(c):
    h, w, ho, wo = c.geom
    return f"{c.path}-{c.src}-{c.dst}-c{c.chan}-{h}x{w}to{ho}x{wo}-m{c.mode}"


# ---------------------------------------------------------------------------
# reference and runner

def case_images(c):
    """The case's batch, dense: (n, h, w, c) or (n, 3, h, w); random bytes, or floats around 100 +- 64."""
    p = PATHS[c.path]
    h, w = c.geom[:2]
    n = batch_of(c)
    shape = (n, 3, h, w) if c.chan == "chw" else (n, h, w, c.chan)
    rng = np.random.default_rng(zlib.crc32(case_id(c).encode()))
    if p.dtype == "u8":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return (rng.standard_normal(shape) * 64 + 100).astype(np.float32)


def ref_image(oracle, p, a, wo, ho, mode, mean, std):
    """The oracle's chain for one image (h, w, c >= 2) or plane (h, w)."""
    if p.interp == "LINEAR":
        r = oracle.resize_linear(a, wo, ho, mode=mode)
    elif p.interp == "CUBIC":
        r = oracle.resize_cubic(oracle.u8_to_f32(a) if a.dtype == np.uint8 else a, wo, ho)
    elif p.interp == "NEAREST":
        r = oracle.resize_nearest(a, wo, ho)
    elif p.interp == "AREA":
        r = oracle.resize_area(a, wo, ho) if p.geoms == "area" else oracle.resize_area_any(a, wo, ho)
    else:
        r = oracle.resize_lanczos4(a, wo, ho)
    if p.out == "norm":
        r = oracle.normalize(oracle.u8_to_f32(r) if r.dtype == np.uint8 else r, mean, std)
    return r


def reference(oracle, p, imgs, layout, wo, ho, mode):
    out = []
    for img in imgs:
        if layout == NHWC:
            c = img.shape[2]
            r = ref_image(oracle, p, img if c > 1 else img[..., 0], wo, ho, mode, MEAN[:c], STD[:c])
            out.append(r.reshape(ho, wo, c))
        else:
            out.append(np.stack([ref_image(oracle, p, pl, wo, ho, mode, MEAN[k:k + 1], STD[k:k + 1])
                                 for k, pl in enumerate(img)]))
    return np.stack(out)


def run_case(ops, dev, oracle, c):
    p = PATHS[c.path]
    layout = NCHW if c.chan == "chw" else NHWC
    ho, wo = c.geom[2:]
    imgs = case_images(c)
    want = reference(oracle, p, imgs, layout, wo, ho, c.mode)
    _, sview = place_as(imgs, dev, layout, c.src, SRC_PLACEMENTS, source=True)
    dbuf, dview = place_as(blank(want.shape, want.dtype), dev, layout, c.dst, DST_PLACEMENTS, source=False)
    nc = 3 if layout == NCHW else c.chan
    with ops.tuning(**p.knobs):
        if p.out == "norm":
            ops.resize_normalize(sview, wo, ho, MEAN[:nc], STD[:nc], interpolation=INTERP[p.interp], mode=c.mode,
                                 layout=layout, out=dview)
        else:
            ops.resize(sview, wo, ho, interpolation=INTERP[p.interp], mode=c.mode, layout=layout, out=dview)
    # the parity bar's one exception: an exact zero's sign in the raw fp32 cubic result
    check_placed(dbuf, dview, want, case_id(c), by_value=p.interp == "CUBIC" and p.out == "same")


def run_path(ops, dev, oracle, path):
    mine = [c for c in CASES if c.path == path]
    assert mine
    for c in mine:
        run_case(ops, dev, oracle, c)


def paths_of(prefix):
    return [p for p in PATHS if p.startswith(prefix)]


# ---------------------------------------------------------------------------
# 1. CPU: the case list's coverage, and a checker that can fail

def test_case_list_covers_every_pair():
    """CASES is a selection, so what it must contain is asserted: every (path,
    source placement) pair the path's type admits, every (path, destination
    placement) pair, every path with 1 to 4 NHWC channels and with NCHW
    planes, NCHW with the dense, odd and padded-plane placements, every shape
    feature the kernels branch on, and the six headline pairs by name."""
    by_path = collections.defaultdict(list)
    for c in CASES:
        assert c.path in PATHS and c.src in SRC_PLACEMENTS and c.dst in DST_PLACEMENTS, c
        assert c.geom in GEOMS[PATHS[c.path].geoms], c
        assert not (NCHW_ONLY & {c.src, c.dst}) or c.chan == "chw", c
        assert c.src not in U8_ONLY or PATHS[c.path].dtype == "u8", c
        by_path[c.path].append(c)
    assert len(CASES) == len(set(CASES)) and len(CASES) < 1000
    for name, p in PATHS.items():
        mine = by_path[name]
        assert {c.src for c in mine} == set(admitted(SRC_PLACEMENTS, p)), name
        assert {c.dst for c in mine} == set(DST_PLACEMENTS), name
        assert {c.chan for c in mine} == set(CHANS), name
    chw = [c for c in CASES if c.chan == "chw"]
    assert {"dense", "odd", "planes"} <= {c.src for c in chw} and {"dense", "odd", "planes"} <= {c.dst for c in chw}
    # the shapes: output widths and heights, 16-multiple output rows and others, the four kinds of scale
    assert {5, 64, 67, 131} <= {c.geom[3] for c in CASES} and {1, 9, 37} <= {c.geom[2] for c in CASES}
    rows16 = {(c.geom[3] * (1 if c.chan == "chw" else c.chan)) % 16 == 0 for c in CASES}
    assert rows16 == {True, False}
    for g, kind in [(GEN[0], "integer down"), (GEN[1], "3:2"), (GEN[3], "up"), (GEN[4], "equal width")]:
        for fam in ("lin_u8", "lin_f32", "cubic", "nearest", "lanczos_u8", "lanczos_f32"):
            assert any(c.geom == g and c.path.startswith(fam) for c in CASES), (kind, fam)
    assert GEN[0][0] % GEN[0][2] == 0 and GEN[0][0] // GEN[0][2] >= 2 and GEN[1][0] * 2 == GEN[1][2] * 3
    assert GEN[3][2] > GEN[3][0] and GEN[3][3] > GEN[3][1] and GEN[4][1] == GEN[4][3] and GEN[4][0] != GEN[4][2]
    assert all(g[1] < 8 for g in NARROW) and WIDE[1] >= 6 * WIDE[3] and WIDE[0] == 24
    assert {(g[1] // g[3], g[0] // g[2]) for g in AREA} == set(AREA_BLOCKS)
    for name in paths_of("area_"):
        assert {(c.geom[1] // c.geom[3], c.geom[0] // c.geom[2]) for c in by_path[name]} == set(AREA_BLOCKS), name
    for name in paths_of("areaany_"):
        assert {c.geom for c in by_path[name]} == set(AREAANY), name

    def has(path, src=None, dst=None, chan=None, mode=None, geom=None):
        return any(c.path == path and src in (None, c.src) and dst in (None, c.dst) and chan in (None, c.chan)
                   and mode in (None, c.mode) and geom in (None, c.geom) for c in CASES)

    # 1. strip x off_p16, c = 1, 3, 4, modes 0, 1, 2
    for path in ("lin_u8_strip1_same", "lin_u8_strip2_same"):
        for ch in (1, 3, 4):
            for mode in (0, 1, 2):
                assert has(path, src="off_p16", chan=ch, mode=mode), (path, ch, mode)
    # 2. NEAREST default and = 1 x img_mis; AREA default and = 3 x img_mis and off4
    for path in ("nearest_u8_default_same", "nearest_u8_row_same", "nearest_f32_default_same", "nearest_f32_row_same"):
        assert has(path, src="img_mis"), path
    # ... by what the selectors do with the placement's own arithmetic, not by name: img_mis reaches them through
    # the image pitch alone and sends an otherwise aligned source to the per-pixel kernel; the same path also
    # runs its row-staged kernel at a dense and at a padded aligned source
    for path in ("nearest_u8_default_same", "nearest_u8_row_same", "nearest_f32_default_same", "nearest_f32_row_same"):
        staged = "row" if "_row_" in path else "wave"
        mis = [c for c in by_path[path] if c.src == "img_mis"]
        assert mis and all((o | r | pl) & 15 == 0 and im & 15 for o, r, pl, im in map(src_pitches, mis)), path
        assert {nearest_kernel(c) for c in mis} == {"pixel"}, path
        for s in ("dense", "p16"):
            assert any(c.src == s and nearest_kernel(c) == staged for c in by_path[path]), (path, s)
    area = {k: [c for c in cases_of("area_u8_") if area_kernel(c) == k]
            for k in ("unit", "lane", "colsum16", "colsum4", "pixel")}

    def blk(c):
        return (c.geom[1] // c.geom[3], c.geom[0] // c.geom[2], 1 if c.chan == "chw" else c.chan)

    for c in AREA_KERNEL_CASES:  # the placements are what the selector's conditions ask for
        off, row, plane, img = src_pitches(c)
        if c.src == "off4":
            assert (off | row | img) & 3 == 0 and (off | row | img) & 15 != 0 and off == 4, c
        elif c.src == "p16":
            assert (off | row | img) & 15 == 0 and row > c.geom[1] * c.chan, c
        elif c.src == "img_mis":
            assert (off | row) & 15 == 0 and img & 15 != 0 and area_kernel(c) == "pixel", c
        elif c.geom[3] == 64:
            assert (off | row | img) & 15 == 0, c
    for path in ("area_u8_default_same", "area_u8_default_norm"):
        for inst in AREA_INSTANCES:
            k = "lane" if inst[0] == 3 and inst[2] >= 3 else "unit"
            for s in ("dense", "p16") + (("off4",) if k == "lane" else ()):
                assert any(c.path == path and c.src == s and blk(c) == inst for c in area[k]), (path, inst, s)
            if k == "unit":  # at a base of 4 mod 16: the dword column sums
                assert any(c.path == path and c.src == "off4" and blk(c) == inst for c in area["colsum4"]), (path, inst)
    for inst in AREA_INSTANCES:  # AREA_KERNEL=3: the 16-byte column sums where aligned, the dword ones at 4 mod 16
        for s, k in (("dense", "colsum16"), ("p16", "colsum16"), ("off4", "colsum4")):
            assert any(c.path == "area_u8_k3_same" and c.src == s and blk(c) == inst for c in area[k]), (inst, s)
    for cc in (3, 4):  # the lane kernel's whole waves (16-byte loads) and partial ones (dword loads)
        per_wave = 64 * (4 if cc == 3 else 1)
        lanes = [c for c in area["lane"] if blk(c)[2] == cc]
        for ay in (3, 2):
            assert any(blk(c)[1] == ay and c.geom[3] >= per_wave for c in lanes), (cc, ay)
            assert any(blk(c)[1] == ay and c.geom[3] % per_wave for c in lanes), (cc, ay)
    assert all(area[k] for k in area)
    assert any(blk(c) == (2, 2, 2) for c in area["unit"]) and any(blk(c) == (2, 2, 2) for c in area["colsum16"])
    # 3. cubic CUBIC_DIRECT = 1 x four destinations with 16-multiple rows; = 2 x p16 with rows that are not
    for d in ("dense", "p16", "off1", "img_mis"):
        assert has("cubic_u8_cd1_same", dst=d, chan=3, geom=GEN[1]) and has("cubic_u8_cd1_norm", dst=d, chan=3, geom=GEN[1])
    assert GEN[1][3] * 3 * 4 % 16 == 0 and GEN[2][3] * 3 * 4 % 16 != 0
    assert has("cubic_u8_cd2_same", dst="p16", chan=3, geom=GEN[2])
    # 4. bilinear gather x p16 destination, 16-multiple rows and not, u8 and normalised
    for path in ("lin_u8_gather_same", "lin_u8_gather_norm"):
        for g in (GEN[0], GEN[2]):
            assert has(path, dst="p16", chan=3, geom=g), (path, g)
    assert GEN[0][3] * 3 % 16 == 0 and GEN[2][3] * 3 % 16 != 0
    # 5. Lanczos, the three knobs and fp32, x sources off1, odd, p16 and destinations off1, odd
    for path in ("lanczos_u8_k0_same", "lanczos_u8_k2_same", "lanczos_u8_k1_same", "lanczos_f32_same"):
        for s in ("off1", "odd", "p16"):
            assert has(path, src=s), (path, s)
        for d in ("off1", "odd"):
            assert has(path, dst=d), (path, d)
    for path in ("lanczos_u8_k0_same", "lanczos_u8_k2_same", "lanczos_u8_k1_same"):
        for ch in (1, 3, 4):
            assert has(path, src="off1", chan=ch, geom=WIDE), (path, ch)
    # 6. staged kernel x sources odd and off1, u8 and fp32, bilinear and cubic
    for path in ("lin_u8_staged_same", "lin_f32_same", "cubic_u8_cd0_same", "cubic_f32_same"):
        for s in ("odd", "off1"):
            assert has(path, src=s), (path, s)


def test_placements_are_what_they_say():
    """The placement tables give the alignments their names promise, for u8
    and fp32: p16 pitches are multiples of 16 bytes with a real pad, img_mis
    and odd leave image 1 off a 16-byte boundary, planes leaves plane 1 off
    one; and the fp32 source helper lays out as `place` does."""
    for es, dt in ((1, np.uint8), (4, np.float32)):
        for layout, shape in ((NHWC, (3, 5, 7, 3)), (NHWC, (3, 4, 16, 1)), (NCHW, (3, 3, 5, 7)), (NCHW, (3, 3, 4, 16))):
            for name, spec in SRC_PLACEMENTS.items():
                if (name in NCHW_ONLY and layout == NHWC) or (name in U8_ONLY and es != 1):
                    continue
                off, rpad, ppad, bpad = pads(spec, layout, shape, es)
                strides, img = strides_of(shape, layout, rpad, ppad, bpad)
                row_b, img_b = strides[1 if layout == NHWC else 2] * es, img * es
                assert off == {"off1": es, "off_p16": es, "off4": 4}.get(name, 0), name
                if spec["row"] == "p16":
                    assert row_b % 16 == 0 and rpad >= 1, (name, shape)
                if name in ("odd", "img_mis"):
                    assert img_b % 16 != 0, (name, shape)
                if name == "img_mis":
                    assert img_b % 16 == 16 - es and row_b % 16 == 0
                if name == "planes":
                    assert (strides[1] * es) % 16 == es and ppad >= 1
    a = (np.arange(2 * 3 * 5 * 2, dtype=np.float32) + 1).reshape(2, 3, 5, 2)
    fbuf, fview = place_f32(a, "cpu", NHWC, 4, 2, 0, 3)
    ubuf, uview = place(a, "cpu", NHWC, off=4, row_pad=2, batch_pad=3)
    assert fview.stride() == uview.stride() and fview.data_ptr() - fbuf.data_ptr() == uview.data_ptr() - ubuf.data_ptr()
    assert np.array_equal(fview.numpy(), a)
    inside = np.zeros(fbuf.numel(), bool)
    np.lib.stride_tricks.as_strided(inside[1:], a.shape, fview.stride())[...] = True
    assert (fbuf.numpy()[~inside] == LOUD).all() and inside.sum() == a.size
    a = a.reshape(2, 2, 3, 5)
    fbuf, fview = place_f32(a, "cpu", NCHW, 0, 1, 2, 3)
    _, uview = place_planes(a, "cpu", off=0, row_pad=1, plane_pad=2, batch_pad=3)
    assert fview.stride() == uview.stride() and np.array_equal(fview.numpy(), a)


def test_checker_can_fail(oracle, monkeypatch):
    """check_placed on CPU tensors: the oracle's result written into a placed
    destination passes; one flipped byte inside the view fails the comparison,
    one in the row padding and one in the batch padding fail the rim check."""
    import torch
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)  # host() reads a CPU tensor as it is
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    want = np.stack([oracle.resize_linear(x, 7, 5) for x in imgs])
    for dt in (np.uint8, np.float32):
        w = want if dt == np.uint8 else np.stack([oracle.normalize(oracle.u8_to_f32(x), MEAN[:3], STD[:3]) for x in want])
        es = w.itemsize
        dbuf, dview = place_as(blank(w.shape, w.dtype), "cpu", NHWC, "odd", DST_PLACEMENTS, source=False)
        off, rpad, _, bpad = pads(DST_PLACEMENTS["odd"], NHWC, w.shape, es)
        assert rpad > 0 and bpad > 0 and (dbuf.numpy() == SENTINEL).all()
        dview.copy_(torch.from_numpy(w))
        check_placed(dbuf, dview, w, "intact")
        row_b = (7 * 3 + rpad) * es
        spots = {"inside the view": off + 2 * row_b + 4 * es, "row padding": off + 2 * row_b + 7 * 3 * es + 1,
                 "batch padding": off + 5 * row_b + 1, "before the view": 0 if off else None,
                 "after the last image": dbuf.numel() - 1}
        for where, pos in spots.items():
            if pos is None:
                continue
            dbuf[pos] ^= 0x40
            with pytest.raises(AssertionError) as e:
                check_placed(dbuf, dview, w, where)
            assert ("bytes differ" in str(e.value)) == (where == "inside the view"), (where, str(e.value))
            assert ("outside the view" in str(e.value)) == (where != "inside the view"), (where, str(e.value))
            dbuf[pos] ^= 0x40
        check_placed(dbuf, dview, w, "restored")
    # the cubic exception is by value and no wider: -0.0 equals 0.0, nothing else passes
    z = np.zeros((1, 2, 2, 1), np.float32)
    dbuf, dview = place_as(blank(z.shape, z.dtype), "cpu", NHWC, "p16", DST_PLACEMENTS, source=False)
    dview.copy_(torch.from_numpy(-z))
    check_placed(dbuf, dview, z, "zero sign", by_value=True)
    with pytest.raises(AssertionError):
        check_placed(dbuf, dview, z, "zero sign, bitwise")
    dview[0, 1, 1, 0] = 1.401298464324817e-45
    with pytest.raises(AssertionError):
        check_placed(dbuf, dview, z, "a denormal is not zero", by_value=True)


# ---------------------------------------------------------------------------
# 2. the paths on the GPU

@gpu
@pytest.mark.parametrize("path", paths_of("lin_u8_"))
def test_bilinear_u8(ops, dev, oracle, path):
    """u8 bilinear, all three fixed-point modes, u8 and normalised output.
    gather: RESIZE_DIRECT=2, resize_direct_kernel (k_resize_direct.hip) for
    every geometry; its stores are 16-byte chunks when the destination base,
    the pitches and the output row bytes are all multiples of 16, else
    narrower ones.  strip1 / strip2: RESIZE_DIRECT=0 with RESIZE_STRIP=1 / 2,
    resize_strip_kernel with 64- / 128-column strips whenever the source row
    pitch is a multiple of 16 -- whatever the base (p16, off_p16, img_mis and
    dense sources whose rows happen to be); any other pitch, or a strip whose
    fetch does not fit, falls back to the staged kernel.  staged: both knobs
    0, resize_kernel (k_resize.hip) through plan_resize.  default: gather for
    one-weighted-row geometries, else strip where it applies, else staged."""
    run_path(ops, dev, oracle, path)


@gpu
@pytest.mark.parametrize("path", paths_of("lin_f32_"))
def test_bilinear_f32(ops, dev, oracle, path):
    """fp32 bilinear: always the staged kernel (k_resize.hip) through
    plan_resize, same-type and normalised output; no fallback."""
    run_path(ops, dev, oracle, path)


@gpu
@pytest.mark.parametrize("path", paths_of("cubic_"))
def test_cubic(ops, dev, oracle, path):
    """Cubic, fp32 and normalised output.  cd1: CUBIC_DIRECT=1, u8 with at
    most 3 interleaved channels runs cubic_cols_kernel (k_cubic_direct.hip)
    when the destination base and its row, plane and image pitches are all
    multiples of 16, otherwise cubic_direct_kernel (the gather kernel); cd2:
    the gather kernel always; cd0: the staged kernel (k_resize.hip).  Four u8
    channels and every fp32 source take the staged kernel whatever the knob."""
    run_path(ops, dev, oracle, path)


@gpu
@pytest.mark.parametrize("path", paths_of("nearest_"))
def test_nearest(ops, dev, oracle, path):
    """INTER_NEAREST (k_pixel.hip), u8 and fp32, same-type and normalised.
    default: the row-per-wave kernel where the source base and all its pitches
    are multiples of 16 and a row is at most a quarter of the staging buffer;
    row: NEAREST_KERNEL=1, the row-per-workgroup kernel under the same
    alignment condition; pixel: NEAREST_KERNEL=0, the per-pixel kernel, which
    is also the fallback of the other two for every misaligned base or pitch
    (off1, off4, odd, img_mis, planes)."""
    run_path(ops, dev, oracle, path)


@gpu
@pytest.mark.parametrize("path", paths_of("area_"))
def test_area_integer_blocks(ops, dev, oracle, path):
    """INTER_AREA with integer blocks 2 x 2, 3 x 3, 4 x 2 and 3 x 2
    (launch_resize_area, k_pixel.hip).  default: area_u8_unit_kernel where the
    source base and pitches are multiples of 16 and area_unit_applies (AX 2 or
    4, or AX 3 with one channel), else area_lane_kernel where they are
    multiples of 4 and area_lane_applies (AX 3 with 3 or 4 channels), else
    the column sums; k3: the 16-byte LDS column sums (dword ones when only
    4-aligned, per-pixel when not even that); k2: dword column sums; k1: the
    per-pixel kernel.  fp32 sources always take the per-pixel kernel.  2 x 2
    blocks round half up for 1, 3 and 4 channels and half to even for 2."""
    run_path(ops, dev, oracle, path)


@gpu
@pytest.mark.parametrize("path", paths_of("areaany_"))
def test_area_any_scale(ops, dev, oracle, path):
    """INTER_AREA at non-integer scales (k_area.hip): area_frac_kernel for the
    down-scale, area_up_kernel for the up-scale and the two mixed scales; one
    kernel each, no alignment-dependent dispatch on the host."""
    run_path(ops, dev, oracle, path)


@gpu
@pytest.mark.parametrize("path", paths_of("lanczos_"))
def test_lanczos(ops, dev, oracle, path):
    """INTER_LANCZOS4 (k_lanczos.hip).  k0: LANCZOS_KERNEL=0, the register-ring
    lanczos_u8_kernel with staged source runs of 1 or 2 16-byte loads per lane
    (run_ni; 0 = per-lane windows where a strip's windows span more than
    2 KiB, as at 9.4:1 with 4 channels); k2: the same kernel with per-lane
    windows; k1: the LDS-ring lanczos_kernel, which every fp32 source takes
    too.  narrow: sources under 8 pixels wide, lanczos_small_kernel whatever
    the knob.  The cached tables carry no pitch or alignment: the same tables
    serve every placement of a geometry here."""
    run_path(ops, dev, oracle, path)


# ---------------------------------------------------------------------------
# 3. refusals

@gpu
def test_refused_placements_write_nothing(ops, dev, oracle):
    """What the resize entry points refuse of a pitched operand.  vacv_resize
    and vacv_resize_normalize with given statistics accept every placement
    (the tests above).  The calls that take statistics of their own output
    read it as one dense range per image: vacv_resize_normalize with mean =
    stddev = NULL, vacv_resize_channel_sums and vacv_resize_mean_stddev give
    VACV_ERR_UNSUPPORTED for a destination with a row pad or a batch pad, for
    every interpolation, and write nothing.  The same calls into a dense
    destination at a byte offset succeed and equal the oracle."""
    rng = np.random.default_rng(91)
    imgs = rng.integers(0, 256, (2, 24, 30, 3), dtype=np.uint8)
    _, sview = place_as(imgs, dev, NHWC, "odd", SRC_PLACEMENTS, source=True)
    for interp, (wo, ho) in [("LINEAR", (17, 11)), ("CUBIC", (17, 11)), ("NEAREST", (17, 11)), ("AREA", (15, 8)),
                             ("AREA", (17, 11)), ("LANCZOS4", (17, 11))]:
        p = Path(interp, "u8", "same", {}, "area" if (wo, ho) == (15, 8) else "areaany")
        raw = reference(oracle, p, imgs, NHWC, wo, ho, 0)
        fdt = np.float32 if interp == "CUBIC" else np.uint8
        calls = [("resize_normalize", np.float32,
                  lambda o: ops.resize_normalize(sview, wo, ho, interpolation=INTERP[interp], out=o)),
                 ("resize_channel_sums", fdt, lambda o: ops.resize_channel_sums(sview, wo, ho, INTERP[interp], out=o)),
                 ("resize_mean_stddev", fdt, lambda o: ops.resize_mean_stddev(sview, wo, ho, INTERP[interp], out=o))]
        for name, dt, fn in calls:
            for d in ("p16", "odd", "img_mis"):
                dbuf, dview = place_as(blank(raw.shape, dt), dev, NHWC, d, DST_PLACEMENTS, source=False)
                unsupported(lambda: fn(dview))
                assert_untouched(dbuf, f"{name} {interp} into {d}")
            dbuf, dview = place_as(blank(raw.shape, dt), dev, NHWC, "off1", DST_PLACEMENTS, source=False)
            fn(dview)
            what = f"{name} {interp} into off1"
            if name != "resize_normalize":
                check_placed(dbuf, dview, raw, what, by_value=interp == "CUBIC")
            elif interp != "CUBIC":  # integer pixels: the kernel's sums are exact, as the oracle's
                want = np.stack([oracle.normalize(x, *oracle.mean_stddev_exact(x)) for x in raw.astype(np.float32)])
                check_placed(dbuf, dview, want, what)
            else:  # statistics of fp32 values depend on the order of the sums: the rim alone
                assert_rim_intact(dbuf, dview, what)
    # the refusal comes before the resize's own argument checks: with a mode that does not exist a pitched
    # destination is still UNSUPPORTED, a dense one INVALID_ARG; neither is written
    import vacv_amd as V
    dbuf, dview = place_as(blank((2, 11, 17, 3), np.uint8), dev, NHWC, "p16", DST_PLACEMENTS, source=False)
    unsupported(lambda: ops.resize_channel_sums(sview, 17, 11, INTERP["LINEAR"], mode=7, out=dview))
    assert_untouched(dbuf, "a pitched destination and an invalid mode")
    dbuf, dview = place_as(blank((2, 11, 17, 3), np.uint8), dev, NHWC, "off1", DST_PLACEMENTS, source=False)
    with pytest.raises(V.VacvError) as e:
        ops.resize_channel_sums(sview, 17, 11, INTERP["LINEAR"], mode=7, out=dview)
    assert e.value.status == V._lib.ERR_INVALID_ARG, e.value.status
    assert_untouched(dbuf, "a dense destination and an invalid mode")


# ---------------------------------------------------------------------------
# 4. cache eviction, release and workspace growth

def _to_dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _evict_roundtrip(run, ref, g0, others, what):
    """G0, then `others` (each checked), then G0 again: the same bits as before and as the oracle."""
    first = host(run(*g0)).copy()
    ref(first, *g0, f"{what} G0")
    for g in others:
        ref(host(run(*g)), *g, f"{what} {g}")
    again = host(run(*g0))
    assert_bits(again, first, f"{what} G0 after the eviction")
    ref(again, *g0, f"{what} G0 after the eviction")


@gpu
def test_plan_cache_eviction(ops, dev, oracle):
    """g_plans is evicted whole when it holds more than 256 plans at an insert
    (resize_plan.cpp:289).  fp32 bilinear always plans: G0 (9 x 11 x 3 -> 7 x
    5), then 260 further geometries from an 8 x 8 source, each against the
    oracle, then G0 again -- rebuilt after the eviction -- gives the first
    run's bits.  Once more with u8 cubic on the staged kernel
    (CUBIC_DIRECT=0), so a second plan kind crosses an eviction."""
    bound = 256  # resize_plan.cpp:289
    outs = [(wo, ho) for wo in range(1, 21) for ho in range(1, 15) if (wo, ho) != (8, 8)][:bound + 4]
    assert len(set(outs)) == bound + 4
    rng = np.random.default_rng(256)
    big, small = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8), rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    for kind in ("f32 bilinear", "u8 cubic"):
        if kind == "f32 bilinear":
            srcs = {9: big.astype(np.float32) * np.float32(0.75) + np.float32(0.125),
                    8: small.astype(np.float32) + np.float32(0.5)}
            interp, knobs = INTERP["LINEAR"], {}
            want = lambda a, wo, ho: oracle.resize_linear(a, wo, ho)
        else:
            srcs, interp, knobs = {9: big, 8: small}, INTERP["CUBIC"], dict(CUBIC_DIRECT=0)
            want = lambda a, wo, ho: oracle.resize_cubic(oracle.u8_to_f32(a), wo, ho)
        devs = {k: _to_dev(v[None], dev) for k, v in srcs.items()}

        def run(h, wo, ho):
            return ops.resize(devs[h], wo, ho, interpolation=interp)

        def ref(got, h, wo, ho, what):  # bits, but for the sign of an exact zero in the cubic result
            (assert_same if kind == "u8 cubic" else assert_bits)(got[0], want(srcs[h], wo, ho).reshape(ho, wo, 3), what)

        with ops.tuning(**knobs):
            _evict_roundtrip(run, ref, (9, 7, 5), [(8, wo, ho) for wo, ho in outs], kind)


@gpu
def test_lanczos_table_eviction(ops, dev, oracle):
    """g_lz_tabs is evicted whole when it holds more than 64 tables at an
    insert (k_lanczos.hip:963): G0 (12 x 16 x 3 -> 9 x 7, wide enough for the
    register-ring kernel), 70 further u8 geometries from an 8 x 8 source, G0
    again."""
    bound = 64  # k_lanczos.hip:963
    outs = [(wo, ho) for wo in range(3, 13) for ho in range(3, 10)][:bound + 6]
    assert len(set(outs)) == bound + 6
    rng = np.random.default_rng(64)
    srcs = {12: rng.integers(0, 256, (12, 16, 3), dtype=np.uint8), 8: rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)}
    devs = {k: _to_dev(v[None], dev) for k, v in srcs.items()}

    def run(h, wo, ho):
        return ops.resize(devs[h], wo, ho, interpolation=INTERP["LANCZOS4"])

    def ref(got, h, wo, ho, what):
        assert_bits(got[0], oracle.resize_lanczos4(srcs[h], wo, ho), what)

    _evict_roundtrip(run, ref, (12, 9, 7), [(8, wo, ho) for wo, ho in outs], "lanczos")


@gpu
def test_area_table_eviction(ops, dev, oracle):
    """g_area_tabs is evicted whole when it holds more than 64 tables at an
    insert (k_area.hip:252): G0 (9 x 11 x 3 -> 7 x 5), 70 further non-integer
    geometries (down, up and mixed) from an 8 x 8 source, G0 again."""
    bound = 64  # k_area.hip:252
    outs = [(wo, ho) for wo in (3, 5, 6, 7, 9, 10, 11, 12, 13, 14) for ho in (3, 5, 6, 7, 9, 10, 11)]
    assert len(set(outs)) == bound + 6 and all(8 % wo and 8 % ho for wo, ho in outs)
    rng = np.random.default_rng(65)
    srcs = {9: rng.integers(0, 256, (9, 11, 3), dtype=np.uint8), 8: rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)}
    devs = {k: _to_dev(v[None], dev) for k, v in srcs.items()}

    def run(h, wo, ho):
        return ops.resize(devs[h], wo, ho, interpolation=INTERP["AREA"])

    def ref(got, h, wo, ho, what):
        assert_bits(got[0], oracle.resize_area_any(srcs[h], wo, ho), what)

    _evict_roundtrip(run, ref, (9, 7, 5), [(8, wo, ho) for wo, ho in outs], "area")


@gpu
def test_release_workspace(ops, dev, oracle):
    """vacv_release_workspace frees the per-stream workspaces -- the column
    kernel's fixed-point accumulators among them, which must read zero when
    they are next allocated -- and the three caches.  Every statistics and
    table user runs, release returns OK, and all of them run again: identical
    bits, the images equal to the oracle.  Release twice in a row is OK."""
    import torch
    rng = np.random.default_rng(1507)
    imgs = rng.integers(0, 256, (3, 40, 50, 3), dtype=np.uint8)
    fl = imgs.astype(np.float32) * np.float32(0.75) + np.float32(0.125)
    src, srcf = _to_dev(imgs, dev), _to_dev(fl, dev)

    def everything():
        res = {}
        for per_image in (True, False):  # 64 x 9 x 3 fp32: 768-byte rows, a dense aligned output -> the column kernel
            out, sums, mean, std = ops.resize_mean_stddev(src, 64, 9, INTERP["CUBIC"], per_image=per_image)
            res[f"cubic per_image={per_image}"] = (out, sums, mean, std)
        res["auto"] = (ops.resize_normalize(src, 33, 21),)
        res["mean_stddev"] = ops.mean_stddev(src)
        res["planned"] = (ops.resize(srcf, 33, 21),)
        res["lanczos"] = (ops.resize(src, 33, 21, interpolation=INTERP["LANCZOS4"]),)
        res["area"] = (ops.resize(src, 33, 21, interpolation=INTERP["AREA"]),)
        torch.cuda.synchronize(dev)
        return {k: [host(t).copy() for t in v] for k, v in res.items()}

    def against_oracle(res):
        want = np.stack([oracle.resize_cubic(oracle.u8_to_f32(x), 64, 9) for x in imgs])
        for per_image in (True, False):
            out, sums, mean, std = res[f"cubic per_image={per_image}"]
            assert_same(out, want, "cubic image")
            exact = want.astype(np.float64).reshape(3, -1, 3)
            exact = exact if per_image else exact.reshape(1, -1, 3)
            s = np.stack([exact.sum(axis=1), (exact * exact).sum(axis=1)], axis=-1)
            assert (np.abs(sums - s) / np.maximum(np.abs(s), 1.0)).max() <= 1e-6  # test_resize_channel_sums' bound
            assert np.abs(mean - exact.mean(axis=1)).max() <= 1e-3
            assert (np.abs(std - exact.std(axis=1)) / exact.std(axis=1)).max() <= 1e-4
        lin = [oracle.resize_linear(x, 33, 21) for x in imgs]
        auto = [oracle.normalize(oracle.u8_to_f32(r), *oracle.mean_stddev_exact(r)) for r in lin]
        assert_bits(res["auto"][0], np.stack(auto), "auto")
        m, s = zip(*[oracle.mean_stddev_exact(x) for x in imgs])
        assert_bits(res["mean_stddev"][0], np.stack(m), "mean")
        assert_bits(res["mean_stddev"][1], np.stack(s), "stddev")
        assert_bits(res["planned"][0], np.stack([oracle.resize_linear(x, 33, 21) for x in fl]), "planned")
        assert_bits(res["lanczos"][0], np.stack([oracle.resize_lanczos4(x, 33, 21) for x in imgs]), "lanczos")
        assert_bits(res["area"][0], np.stack([oracle.resize_area_any(x, 33, 21) for x in imgs]), "area")

    before = everything()
    against_oracle(before)
    ops.release_workspace()  # raises unless VACV_OK
    after = everything()
    for k in before:
        for a, b in zip(before[k], after[k]):
            assert_bits(b, a, f"{k} after release")
    against_oracle(after)
    ops.release_workspace()
    ops.release_workspace()
    again = everything()
    for k in before:
        for a, b in zip(before[k], again[k]):
            assert_bits(b, a, f"{k} after two releases")


@gpu
def test_workspace_growth(ops, dev, oracle):
    """The workspace's grow path (vacv_abi.cpp, workspace(): synchronise,
    free, reallocate).  Its minimum capacity is 1 MiB = 1,048,576 bytes, and
    the one request of the resize family that can exceed it at the smallest
    batch is vacv_resize_channel_sums' partials for the cubic gather kernel,
    n * groups * 2 * c doubles with groups = ceil(w * h / 512)
    (cubic_sums_groups_bound; per_image_stats and vacv_channel_sums ask for
    at most 2048 blocks * 2 * 4 * 8 = 131,072 bytes).  With n = 1 and c = 3
    that is 48 bytes per group, more than 1 MiB from 21,846 groups on: a
    3346 x 3346 output has ceil(11,195,716 / 512) = 21,867 groups =
    1,049,616 bytes.  Its rows are 40,152 bytes, not a multiple of 16, so the
    gather kernel runs and writes its partials all over the grown buffer.
    Device memory: the 134,348,592-byte fp32 output, once (the separately
    resized output reuses the buffer), a 192-byte source and the 1 MiB
    workspace: under 140 MB.

    After a release, a small request (1 MiB allocated), the large one (the
    grow path), and the small one again: each fused result is within 1e-6
    relative of vacv_channel_sums of the separately resized output (the bound
    of test_resize_channel_sums), repeats have equal bits, and the fused and
    the separate output are the same image (equal sums of their bit patterns
    and bit-identical vacv_channel_sums)."""
    import torch
    import re
    from conftest import PKG
    side = 3346
    # cubic_sums_groups_bound (k_cubic_direct.hip:673-676): ceil(w * h / (4 * kWavePx)), kWavePx = 64 * kPxl
    kpxl = int(re.search(r"constexpr int kPxl = (\d+);", (PKG / "csrc" / "k_cubic_direct.hip").read_text()).group(1))
    assert 4 * 64 * kpxl == 512, "the groups bound changed: choose `side` again so that the request exceeds 1 MiB"
    groups = -(-side * side // 512)
    assert groups * 2 * 3 * 8 > 1 << 20 and (side * 3 * 4) % 16 != 0 and side * side * 12 < 140e6
    rng = np.random.default_rng(128)
    src = _to_dev(rng.integers(0, 256, (1, 8, 8, 3), dtype=np.uint8), dev)
    cubic = INTERP["CUBIC"]

    def rel(a, b):
        return ((a - b).abs() / b.abs().clamp(min=1.0)).max().item()

    def small():
        out, sums = ops.resize_channel_sums(src, 61, 37, cubic)  # 732-byte rows: the gather kernel, 5 groups
        ref = ops.resize(src, 61, 37, interpolation=cubic)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
        assert rel(sums, ops.channel_sums(ref)) <= 1e-6
        return sums.clone()

    ops.release_workspace()
    s0 = small()
    buf = torch.empty((1, side, side, 3), dtype=torch.float32, device=dev)
    _, big1 = ops.resize_channel_sums(src, side, side, cubic, out=buf)
    big1 = big1.clone()
    digest1 = buf.view(torch.int32).sum(dtype=torch.int64).item()
    own1 = ops.channel_sums(buf).clone()
    _, big2 = ops.resize_channel_sums(src, side, side, cubic, out=buf)
    assert torch.equal(big2, big1), "the large request, repeated"
    ops.resize(src, side, side, interpolation=cubic, out=buf)  # the separately resized output
    want = ops.channel_sums(buf)
    torch.cuda.synchronize(dev)
    assert buf.view(torch.int32).sum(dtype=torch.int64).item() == digest1 and torch.equal(want, own1)
    assert rel(big1, want) <= 1e-6
    s1 = small()
    assert torch.equal(s1, s0), "the small request after the growth"
    del buf
    torch.cuda.empty_cache()
    ops.release_workspace()
    assert torch.equal(small(), s0), "the small request after a release"


@gpu
def test_non_default_stream(ops, dev, oracle):
    """One call per interpolation on a fresh stream, the source produced on
    that stream, at geometries no other test uses: the plan or table of a
    geometry is uploaded on the calling stream and synchronised, so that any
    stream may use it next -- the same call then runs on the default stream.
    Compared with the oracle after vacv_stream_synchronize."""
    import torch
    import vacv_amd as V
    rng = np.random.default_rng(77)
    imgs = rng.integers(0, 256, (2, 23, 29, 3), dtype=np.uint8)
    fl = imgs.astype(np.float32) * np.float32(0.5) + np.float32(3.25)
    wo, ho = 19, 13
    calls = [("LINEAR", imgs, lambda a: oracle.resize_linear(a, wo, ho)),
             ("LINEAR", fl, lambda a: oracle.resize_linear(a, wo, ho)),
             ("CUBIC", imgs, lambda a: oracle.resize_cubic(oracle.u8_to_f32(a), wo, ho)),
             ("CUBIC", fl, lambda a: oracle.resize_cubic(a, wo, ho)),
             ("NEAREST", imgs, lambda a: oracle.resize_nearest(a, wo, ho)),
             ("AREA", imgs, lambda a: oracle.resize_area_any(a, wo, ho)),
             ("LANCZOS4", imgs, lambda a: oracle.resize_lanczos4(a, wo, ho))]
    stream = torch.cuda.Stream(device=dev)
    for interp, a, ref in calls:
        want = np.stack([ref(x) for x in a])
        with torch.cuda.stream(stream):
            src = torch.from_numpy(a).to(dev, non_blocking=True)
            src = src + 0 if a.dtype == np.float32 else src ^ 0  # produced by a kernel of this stream
            out = ops.resize(src, wo, ho, interpolation=INTERP[interp], stream=stream)
        assert V._lib.load().vacv_stream_synchronize(stream.cuda_stream) == V._lib.OK
        got = out.cpu().numpy()
        assert_same(got, want, f"{interp} {a.dtype} on a second stream")
        if interp != "CUBIC":
            assert_bits(got, want, f"{interp} {a.dtype} on a second stream")
        src0 = _to_dev(a, dev)
        again = host(ops.resize(src0, wo, ho, interpolation=INTERP[interp]))
        assert_bits(again, got, f"{interp} then on the default stream")
