#!/usr/bin/env python3
"""Kernel micro-bench for profiling (rocprofv3 wraps this; no CPU work).

  python tools/kbench.py --op resize_normalize --iters 20
Prints one JSON line per op: average launch time from HIP events and the
algorithmic GB/s (vacv_amd.roofline)."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "arm-neon-opencv_amd"))

MEAN = [103.94, 116.78, 123.68]
STD = [57.375, 57.12, 58.395]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", default="resize_normalize")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--only", default="", help="run only the cases whose name contains this")
    ap.add_argument("--sweep", default="",
                    help="kernel-variant knobs (VACV_TUNE_*, vacv_set_tuning) to sweep, "
                         "e.g. 'DIRECT_ALIGN=0,1;RESIZE_WORK=2,4'")
    ap.add_argument("--compare", action="store_true",
                    help="--op warp_rois: time each one-call case against the same crops as a loop of single "
                         "calls (vacv_warp_affine; vacv_warp_affine_normalize + one vacv_change_layout), alternating "
                         "(the standardize case: against warp_affine_rois + normalize(NULL, NULL) + change_layout); "
                         "--op yuv_rois: against vacv_cvt_color of all frames + vacv_warp_affine_rois[_normalize] "
                         "(the standardize case: + vacv_warp_affine_rois_standardize); "
                         "--op crop_resize_rois: against a loop of vacv_crop + vacv_resize[_normalize] single calls "
                         "(the standardize case: against crop_resize_rois + normalize(NULL, NULL) + change_layout); "
                         "--op yuv_crop_resize_rois: against vacv_cvt_color of all frames + "
                         "vacv_crop_resize_rois[_normalize] (the standardize case: + "
                         "vacv_crop_resize_rois_standardize); "
                         "--op yuv_match_rois: against vacv_cvt_color of all frames + vacv_match_template_rois")
    ap.add_argument("--baseline-lib", default="",
                    help="--compare: libvacv_hip.so of another build (e.g. the parent commit's) to run the loop on; "
                         "default: this build's own single-call entry points")
    a = ap.parse_args()
    import torch
    import vacv_amd
    from vacv_amd import ops
    from vacv_amd.roofline import resize_bytes
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(1)

    def frames(n, h, w, c=3):
        return torch.randint(0, 256, (n, h, w, c), dtype=torch.uint8, device=dev, generator=g)

    cases = {}
    if a.op in ("resize_normalize", "all"):
        n = a.batch or 256
        src = frames(n, 1080, 1920)
        out = torch.empty((n, 360, 640, 3), dtype=torch.float32, device=dev)
        cases["resize_normalize_1080p_640x360"] = (lambda src=src, out=out: ops.resize_normalize(src, 640, 360, MEAN, STD, out=out),
                                                   n * resize_bytes(1920, 1080, 3, 640, 360, 1, 4), n * 1920 * 1080)
    if a.op in ("resize", "all"):
        n = a.batch or 256
        src = frames(n, 1080, 1920)
        o1 = torch.empty((n, 360, 640, 3), dtype=torch.uint8, device=dev)
        o2 = torch.empty((n, 720, 1280, 3), dtype=torch.uint8, device=dev)
        cases["resize_1080p_640x360_u8"] = (lambda src=src, o1=o1: ops.resize(src, 640, 360, out=o1),
                                            n * resize_bytes(1920, 1080, 3, 640, 360, 1, 1), n * 1920 * 1080)
        cases["resize_1080p_1280x720_u8"] = (lambda src=src, o2=o2: ops.resize(src, 1280, 720, out=o2),
                                             n * resize_bytes(1920, 1080, 3, 1280, 720, 1, 1), n * 1920 * 1080)
    if a.op in ("resize_other", "all"):
        # INTER_NEAREST / INTER_AREA (OpenCV-delegated modes): read the frame, write the output
        n = a.batch or 256
        src = frames(n, 1080, 1920)
        o3 = torch.empty((n, 360, 640, 3), dtype=torch.uint8, device=dev)
        o2 = torch.empty((n, 540, 960, 3), dtype=torch.uint8, device=dev)
        cases["area_1080p_640x360_u8"] = (
            lambda src=src, o=o3: ops.resize(src, 640, 360, interpolation=vacv_amd.INTER_AREA, out=o),
            n * (1920 * 1080 * 3 + 640 * 360 * 3), n * 1920 * 1080)
        cases["area_1080p_960x540_u8"] = (
            lambda src=src, o=o2: ops.resize(src, 960, 540, interpolation=vacv_amd.INTER_AREA, out=o),
            n * (1920 * 1080 * 3 + 960 * 540 * 3), n * 1920 * 1080)
        # nearest reads one pixel in (1920/640)^2 = 9 (whole 64 B lines of them, all of 1 in 3 rows)
        cases["nearest_1080p_640x360_u8"] = (
            lambda src=src, o=o3: ops.resize(src, 640, 360, interpolation=vacv_amd.INTER_NEAREST, out=o),
            n * (360 * 1920 * 3 + 640 * 360 * 3), n * 1920 * 1080)
    if a.op in ("lanczos", "all"):
        # INTER_LANCZOS4: every source row is weighted (8 taps at a 3x downscale)
        n = a.batch or 256
        src = frames(n, 1080, 1920)
        o3 = torch.empty((n, 360, 640, 3), dtype=torch.uint8, device=dev)
        cases["lanczos_1080p_640x360_u8"] = (
            lambda src=src, o=o3: ops.resize(src, 640, 360, interpolation=vacv_amd.INTER_LANCZOS4, out=o),
            n * (1920 * 1080 * 3 + 640 * 360 * 3), n * 1920 * 1080)
        of = torch.empty((n, 360, 640, 3), dtype=torch.float32, device=dev)
        cases["lanczos_normalize_1080p_640x360"] = (
            lambda src=src, o=of: ops.resize_normalize(src, 640, 360, MEAN, STD, interpolation=vacv_amd.INTER_LANCZOS4,
                                                       out=o),
            n * (1920 * 1080 * 3 + 640 * 360 * 12), n * 1920 * 1080)
    if a.op in ("warp", "all"):
        n = a.batch or 128
        src = frames(n, 720, 1280)
        o = torch.empty_like(src)
        m = ops.rotation_matrix(0.9, 15.0, (640, 360, 640, 360))
        cases["warp_720p_rot15_u8"] = (lambda src=src, m=m, o=o: ops.warp_affine(src, m, 1280, 720, out=o), n * 2 * 1280 * 720 * 3,
                                       n * 1280 * 720)
        for rot in (0.0, 5.0, 45.0):
            mr = ops.rotation_matrix(0.9, rot, (640, 360, 640, 360))
            cases[f"warp_720p_rot{int(rot)}_u8"] = (lambda src=src, m=mr, o=o: ops.warp_affine(src, m, 1280, 720, out=o),
                                                   n * 2 * 1280 * 720 * 3, n * 1280 * 720)
        # INTER_NEAREST (OpenCV's fixed-point map): the source pixels it reads, ~1/0.81 of a frame at scale 0.9
        cases["warp_nearest_720p_rot15_u8"] = (
            lambda src=src, m=m, o=o: ops.warp_affine(src, m, 1280, 720, flags=vacv_amd.INTER_NEAREST, out=o),
            n * 2 * 1280 * 720 * 3, n * 1280 * 720)
        of = torch.empty((n, 720, 1280, 3), dtype=torch.float32, device=dev)
        cases["warp_normalize_720p_rot15"] = (lambda src=src, m=m, of=of: ops.warp_affine_normalize(src, m, 1280, 720, MEAN, STD, out=of),
                                              n * 5 * 1280 * 720 * 3, n * 1280 * 720)
    if a.op in ("cvt", "all"):
        n = a.batch or 256
        yuv = torch.randint(0, 256, (n, 1620, 1920), dtype=torch.uint8, device=dev, generator=g)
        o = torch.empty((n, 1080, 1920, 3), dtype=torch.float32, device=dev)
        cases["nv21_bgr_normalize_1080p"] = (lambda yuv=yuv, o=o: ops.cvt_color_normalize(yuv, mean=MEAN, std=STD, out=o),
                                             n * (1920 * 1620 + 1920 * 1080 * 12), n * 1920 * 1080)
    if a.op in ("cvt_cv", "all"):
        # the OpenCV colour codes (k_color_cv.hip): YUV420 in, 3 or 4 channels out; gray -> BGR
        n = a.batch or 256
        yuv = torch.randint(0, 256, (n, 1620, 1920), dtype=torch.uint8, device=dev, generator=g)
        o4 = torch.empty((n, 1080, 1920, 4), dtype=torch.uint8, device=dev)
        o3 = torch.empty((n, 1080, 1920, 3), dtype=torch.uint8, device=dev)
        cases["nv21_bgra_1080p"] = (lambda yuv=yuv, o=o4: ops.cvt_color(yuv, vacv_amd.COLOR_YUV2BGRA_NV21, out=o),
                                    n * (1920 * 1620 + 1920 * 1080 * 4), n * 1920 * 1080)
        cases["yv12_bgr_1080p"] = (lambda yuv=yuv, o=o3: ops.cvt_color(yuv, vacv_amd.COLOR_YUV2BGR_YV12, out=o),
                                   n * (1920 * 1620 + 1920 * 1080 * 3), n * 1920 * 1080)
        gray = yuv[:, :1080]
        cases["gray_bgr_1080p"] = (lambda g_=gray, o=o3: ops.cvt_color(g_, vacv_amd.COLOR_GRAY2BGR, out=o),
                                   n * 1920 * 1080 * 4, n * 1920 * 1080)
    if a.op in ("yuv_resize", "all"):
        from vacv_amd.roofline import yuv_resize_bytes
        n = a.batch or 256
        yuv = torch.randint(0, 256, (n, 1620, 1920), dtype=torch.uint8, device=dev, generator=g)
        o1 = torch.empty((n, 3, 360, 640), dtype=torch.float32, device=dev)
        o2 = torch.empty((n, 3, 224, 224), dtype=torch.float32, device=dev)
        cases["nv21_resize_normalize_1080p_640x360_chw"] = (
            lambda yuv=yuv, o1=o1: ops.cvt_color_resize_normalize(yuv, 640, 360, MEAN, STD, out=o1),
            n * yuv_resize_bytes(1920, 1080, 640, 360), n * 1920 * 1080)
        o3 = torch.empty((n, 360, 640, 3), dtype=torch.float32, device=dev)
        cases["nv21_resize_normalize_1080p_640x360_hwc"] = (
            lambda yuv=yuv, o3=o3: ops.cvt_color_resize_normalize(yuv, 640, 360, MEAN, STD, layout=vacv_amd.NHWC, out=o3),
            n * yuv_resize_bytes(1920, 1080, 640, 360), n * 1920 * 1080)
        o4 = torch.empty((n, 360, 640, 3), dtype=torch.uint8, device=dev)
        cases["nv21_resize_1080p_640x360_u8"] = (
            lambda yuv=yuv, o4=o4: ops.cvt_color_resize(yuv, 640, 360, out=o4),
            n * yuv_resize_bytes(1920, 1080, 640, 360, out_esize=1), n * 1920 * 1080)
        cases["nv21_resize_normalize_1080p_224_chw"] = (
            lambda yuv=yuv, o2=o2: ops.cvt_color_resize_normalize(yuv, 224, 224, MEAN, STD, out=o2),
            n * yuv_resize_bytes(1920, 1080, 224, 224), n * 1920 * 1080)
    if a.op in ("cubic", "all"):
        n = a.batch or 128
        src = frames(n, 1440, 2560)
        o = torch.empty((n, 224, 224, 3), dtype=torch.float32, device=dev)
        cases["cubic_1440p_224_u8_f32"] = (lambda src=src, o=o: ops.resize(src, 224, 224, interpolation=vacv_amd.INTER_CUBIC, out=o),
                                           n * resize_bytes(2560, 1440, 3, 224, 224, 1, 4, cubic=True), n * 2560 * 1440)
        cases["cubic_stats_1440p_224"] = (
            lambda src=src, o=o: ops.resize_mean_stddev(src, 224, 224, interpolation=vacv_amd.INTER_CUBIC,
                                                        per_image=False, out=o),
            n * resize_bytes(2560, 1440, 3, 224, 224, 1, 4, cubic=True), n * 2560 * 1440)
    if a.op in ("match", "all"):
        # correlation MACs: (W-w+1)(H-h+1) * w*h*c; bytes: image + result
        n = a.batch or 8
        src = frames(n, 720, 1280)
        tpl = frames(1, 64, 64)[0]
        o = torch.empty((n, 720 - 63, 1280 - 63), dtype=torch.float32, device=dev)
        for m, name in ((2, "ccorr"), (5, "ccoeff_normed")):
            cases[f"match_720p_64x64_{name}"] = (lambda src=src, tpl=tpl, o=o, m=m: ops.match_template(src, tpl, m, out=o),
                                                 n * (1280 * 720 * 3 + 657 * 1217 * 4), n * 1280 * 720)
        # GMAC/s of the correlation, for its compute roofline (v_dot4_u32_u8)
        macs = n * 657 * 1217 * 64 * 64 * 3
        cases["match_720p_64x64_ccorr_macs"] = (lambda src=src, tpl=tpl, o=o: ops.match_template(src, tpl, 2, out=o),
                                                macs, n * 1280 * 720)
    if a.op in ("dtype", "all", "calib"):
        n = a.batch or 64
        src = frames(n, 1080, 1920)
        o = torch.empty((n, 1080, 1920, 3), dtype=torch.float32, device=dev)
        cases["u8_to_f32_1080p"] = (lambda src=src, o=o: ops.change_dtype(src, torch.float32, out=o) if False else
                                    ops.change_dtype(src, torch.float32), n * 1920 * 1080 * 15, n * 1920 * 1080)
    if a.op in ("layout", "all"):
        n = a.batch or 256
        src = frames(n, 360, 640)
        cases["hwc_to_chw_640x360_u8"] = (lambda src=src: ops.change_layout(src, vacv_amd.NCHW),
                                          n * 640 * 360 * 6, n * 640 * 360)
    loops, std_chains = {}, {}
    if a.op in ("warp_rois", "all"):
        # many small crops, each with its own matrix, in ONE launch
        # (vacv_warp_affine_rois): seeded geometry -- rotation uniform in +-30
        # degrees, a source footprint of ~250 px per side, centres anywhere in
        # the frame (so some crops hang partly off it)
        import numpy as np
        from vacv_amd.roofline import warp_rois_bytes
        rng = np.random.default_rng(20261019)

        def roi_maps(n, fw, fh, wo, ho, foot=250.0):
            ms = np.zeros((n, 6), np.float32)
            for i in range(n):
                ang, s = np.deg2rad(rng.uniform(-30.0, 30.0)), max(wo, ho) / foot
                cx, cy = rng.uniform(0, fw), rng.uniform(0, fh)
                ca, sa = s * np.cos(ang), s * np.sin(ang)
                ms[i] = [ca, sa, wo / 2 - ca * cx - sa * cy, -sa, ca, ho / 2 + sa * cx - ca * cy]
            return ms

        src = frames(8, 1080, 1920)
        ms = roi_maps(256, 1920, 1080, 112, 112)
        idx = np.arange(256, dtype=np.int32) % 8
        dms, didx = torch.from_numpy(ms).to(dev), torch.from_numpy(idx).to(dev)
        o = torch.empty((256, 112, 112, 3), dtype=torch.uint8, device=dev)
        cases["warp_rois_1080p_256x112_u8"] = (
            lambda src=src, dms=dms, didx=didx, o=o: ops.warp_affine_rois(src, dms, 112, 112, src_index=didx, out=o),
            warp_rois_bytes(1920, 1080, 3, 112, 112, ms), 256 * 112 * 112)
        loops["warp_rois_1080p_256x112_u8"] = dict(src=src, ms=ms, idx=idx, out=torch.empty_like(o), norm=False)
        of = torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev)
        cases["warp_rois_normalize_1080p_256x112_chw"] = (
            lambda src=src, dms=dms, didx=didx, of=of: ops.warp_affine_rois_normalize(
                src, dms, 112, 112, MEAN, STD, src_index=didx, out_layout=vacv_amd.NCHW, out=of),
            warp_rois_bytes(1920, 1080, 3, 112, 112, ms, out_esize=4), 256 * 112 * 112)
        loops["warp_rois_normalize_1080p_256x112_chw"] = dict(src=src, ms=ms, idx=idx, out=torch.empty_like(of),
                                                              norm=True)
        # the reference harness's crop size: 64 crops of one 1280 x 720 frame
        src7 = frames(1, 720, 1280)
        ms7 = roi_maps(64, 1280, 720, 140, 210)
        dms7 = torch.from_numpy(ms7).to(dev)
        o7 = torch.empty((64, 210, 140, 3), dtype=torch.uint8, device=dev)
        cases["warp_rois_720p_64x140x210_u8"] = (
            lambda src7=src7, dms7=dms7, o7=o7: ops.warp_affine_rois(src7, dms7, 140, 210, out=o7),
            warp_rois_bytes(1280, 720, 3, 140, 210, ms7), 64 * 140 * 210)
        loops["warp_rois_720p_64x140x210_u8"] = dict(src=src7, ms=ms7, idx=np.zeros(64, np.int32),
                                                     out=torch.empty_like(o7), norm=False)
        # the 1080p maps, each crop standardized by its own statistics
        # (vacv_warp_affine_rois_standardize); the comparator is the chain it
        # replaces, into preallocated buffers
        from vacv_amd.roofline import warp_affine_rois_standardize_bytes
        os_ = torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev)
        cases["warp_rois_standardize_1080p_256x112_chw"] = (
            lambda src=src, dms=dms, didx=didx, os_=os_: ops.warp_affine_rois_standardize(
                src, dms, 112, 112, src_index=didx, layout=vacv_amd.NCHW, out=os_),
            warp_affine_rois_standardize_bytes(1920, 1080, 3, 112, 112, ms), 256 * 112 * 112)
        std_chains["warp_rois_standardize_1080p_256x112_chw"] = dict(
            frames=8, out=torch.empty_like(os_),
            u8=lambda u, src=src, dms=dms, didx=didx: ops.warp_affine_rois(src, dms, 112, 112, src_index=didx, out=u))
    chains = {}
    if a.op in ("yuv_rois", "all"):
        # the warp_rois cases with NV21 frames as the source
        # (vacv_cvt_color_warp_affine_rois): the same seeded geometry
        import numpy as np
        from vacv_amd.roofline import yuv_warp_rois_bytes
        rng = np.random.default_rng(20261019)

        def yuv_roi_maps(n, fw, fh, wo, ho, foot=250.0):
            ms = np.zeros((n, 6), np.float32)
            for i in range(n):
                ang, s = np.deg2rad(rng.uniform(-30.0, 30.0)), max(wo, ho) / foot
                cx, cy = rng.uniform(0, fw), rng.uniform(0, fh)
                ca, sa = s * np.cos(ang), s * np.sin(ang)
                ms[i] = [ca, sa, wo / 2 - ca * cx - sa * cy, -sa, ca, ho / 2 + sa * cx - ca * cy]
            return ms

        yuv = torch.randint(0, 256, (8, 1620, 1920), dtype=torch.uint8, device=dev, generator=g)
        ms = yuv_roi_maps(256, 1920, 1080, 112, 112)
        idx = np.arange(256, dtype=np.int32) % 8
        dms, didx = torch.from_numpy(ms).to(dev), torch.from_numpy(idx).to(dev)
        o = torch.empty((256, 112, 112, 3), dtype=torch.uint8, device=dev)
        cases["yuv_rois_1080p_256x112_u8"] = (
            lambda yuv=yuv, dms=dms, didx=didx, o=o: ops.cvt_color_warp_affine_rois(yuv, dms, 112, 112, src_index=didx,
                                                                                  out=o),
            yuv_warp_rois_bytes(1920, 1080, 112, 112, ms), 256 * 112 * 112)
        chains["yuv_rois_1080p_256x112_u8"] = dict(yuv=yuv, ms=dms, idx=didx, out=torch.empty_like(o), norm=False)
        of = torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev)
        cases["yuv_rois_normalize_1080p_256x112_chw"] = (
            lambda yuv=yuv, dms=dms, didx=didx, of=of: ops.cvt_color_warp_affine_rois_normalize(
                yuv, dms, 112, 112, MEAN, STD, src_index=didx, layout=vacv_amd.NCHW, out=of),
            yuv_warp_rois_bytes(1920, 1080, 112, 112, ms, out_esize=4), 256 * 112 * 112)
        chains["yuv_rois_normalize_1080p_256x112_chw"] = dict(yuv=yuv, ms=dms, idx=didx, out=torch.empty_like(of),
                                                              norm=True)
        # the reference harness's crop size: 64 crops of one 1280 x 720 frame
        yuv7 = torch.randint(0, 256, (1, 1080, 1280), dtype=torch.uint8, device=dev, generator=g)
        ms7 = yuv_roi_maps(64, 1280, 720, 140, 210)
        dms7 = torch.from_numpy(ms7).to(dev)
        o7 = torch.empty((64, 210, 140, 3), dtype=torch.uint8, device=dev)
        cases["yuv_rois_720p_64x140x210_u8"] = (
            lambda yuv7=yuv7, dms7=dms7, o7=o7: ops.cvt_color_warp_affine_rois(yuv7, dms7, 140, 210, out=o7),
            yuv_warp_rois_bytes(1280, 720, 140, 210, ms7), 64 * 140 * 210)
        chains["yuv_rois_720p_64x140x210_u8"] = dict(yuv=yuv7, ms=dms7, idx=None, out=torch.empty_like(o7), norm=False)
        # the 1080p maps, each crop standardized by its own statistics
        # (vacv_cvt_color_warp_affine_rois_standardize); the comparator is the
        # chain it replaces: cvt_color of all frames, then the BGR standardize
        # call, into preallocated buffers
        from vacv_amd.roofline import yuv_warp_rois_standardize_bytes
        os_ = torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev)
        bgr, oc = torch.empty((8, 1080, 1920, 3), dtype=torch.uint8, device=dev), torch.empty_like(os_)

        def warp_std_chain(yuv=yuv, dms=dms, didx=didx, bgr=bgr, oc=oc):
            ops.cvt_color(yuv, out=bgr)
            ops.warp_affine_rois_standardize(bgr, dms, 112, 112, src_index=didx, layout=vacv_amd.NCHW, out=oc)

        cases["yuv_rois_standardize_1080p_256x112_chw"] = (
            lambda yuv=yuv, dms=dms, didx=didx, os_=os_: ops.cvt_color_warp_affine_rois_standardize(
                yuv, dms, 112, 112, src_index=didx, layout=vacv_amd.NCHW, out=os_),
            yuv_warp_rois_standardize_bytes(1920, 1080, 112, 112, ms), 256 * 112 * 112)
        std_chains["yuv_rois_standardize_1080p_256x112_chw"] = dict(frames=8, out=oc, chain=warp_std_chain)
    crop_loops = {}
    if a.op in ("crop_resize_rois", "all"):
        # many upright crops, each with its own rect, in ONE launch
        # (vacv_crop_resize_rois): seeded boxes of 32..400 pixels per side
        # anywhere inside the frame, mirroring the warp_rois cases
        import numpy as np
        from vacv_amd.roofline import crop_resize_rois_bytes
        rng = np.random.default_rng(20261020)

        def roi_rects(n, fw, fh, lo=32, hi=400):
            wh = rng.integers(lo, hi + 1, (n, 2))
            lt = (rng.random((n, 2)) * (np.array([fw, fh]) - wh + 1)).astype(np.int64)
            return np.concatenate([lt, wh], 1).astype(np.int32)

        src = frames(8, 1080, 1920)
        rects = roi_rects(256, 1920, 1080)
        idx = np.arange(256, dtype=np.int32) % 8
        drects, didx = torch.from_numpy(rects).to(dev), torch.from_numpy(idx).to(dev)
        o = torch.empty((256, 112, 112, 3), dtype=torch.uint8, device=dev)
        cases["crop_resize_rois_1080p_256x112_u8"] = (
            lambda src=src, drects=drects, didx=didx, o=o: ops.crop_resize_rois(src, drects, 112, 112, src_index=didx,
                                                                               out=o),
            crop_resize_rois_bytes(3, 1, 112, 112, rects, 1), 256 * 112 * 112)
        crop_loops["crop_resize_rois_1080p_256x112_u8"] = dict(src=src, rects=rects, idx=idx, out=torch.empty_like(o),
                                                               norm=False)
        of = torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev)
        cases["crop_resize_rois_normalize_1080p_256x112_chw"] = (
            lambda src=src, drects=drects, didx=didx, of=of: ops.crop_resize_rois_normalize(
                src, drects, 112, 112, MEAN, STD, src_index=didx, layout=vacv_amd.NCHW, out=of),
            crop_resize_rois_bytes(3, 1, 112, 112, rects, 4), 256 * 112 * 112)
        crop_loops["crop_resize_rois_normalize_1080p_256x112_chw"] = dict(src=src, rects=rects, idx=idx,
                                                                          out=torch.empty_like(of), norm=True)
        # the reference harness's crop size: 64 crops of one 1280 x 720 frame
        src7 = frames(1, 720, 1280)
        rects7 = roi_rects(64, 1280, 720)
        drects7 = torch.from_numpy(rects7).to(dev)
        o7 = torch.empty((64, 210, 140, 3), dtype=torch.uint8, device=dev)
        cases["crop_resize_rois_720p_64x140x210_u8"] = (
            lambda src7=src7, drects7=drects7, o7=o7: ops.crop_resize_rois(src7, drects7, 140, 210, out=o7),
            crop_resize_rois_bytes(3, 1, 140, 210, rects7, 1), 64 * 140 * 210)
        crop_loops["crop_resize_rois_720p_64x140x210_u8"] = dict(src=src7, rects=rects7, idx=np.zeros(64, np.int32),
                                                                 out=torch.empty_like(o7), norm=False)
        # the same boxes, each crop standardized by its own statistics
        # (vacv_crop_resize_rois_standardize); the comparator is the chain it
        # replaces, into preallocated buffers
        from vacv_amd.roofline import crop_resize_rois_standardize_bytes
        os_ = torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev)
        cases["crop_resize_rois_standardize_1080p_256x112_chw"] = (
            lambda src=src, drects=drects, didx=didx, os_=os_: ops.crop_resize_rois_standardize(
                src, drects, 112, 112, src_index=didx, layout=vacv_amd.NCHW, out=os_),
            crop_resize_rois_standardize_bytes(3, 112, 112, rects, False, 1920, 1080), 256 * 112 * 112)
        std_chains["crop_resize_rois_standardize_1080p_256x112_chw"] = dict(
            frames=8, out=torch.empty_like(os_),
            u8=lambda u, src=src, drects=drects, didx=didx: ops.crop_resize_rois(src, drects, 112, 112, src_index=didx,
                                                                                out=u))
    crop_chains = {}
    if a.op in ("yuv_crop_resize_rois", "all"):
        # the crop_resize_rois cases with NV21 frames as the source
        # (vacv_cvt_color_crop_resize_rois): the same seeded boxes
        import numpy as np
        from vacv_amd.roofline import yuv_crop_resize_rois_bytes
        rng = np.random.default_rng(20261020)

        def yuv_roi_rects(n, fw, fh, lo=32, hi=400):
            wh = rng.integers(lo, hi + 1, (n, 2))
            lt = (rng.random((n, 2)) * (np.array([fw, fh]) - wh + 1)).astype(np.int64)
            return np.concatenate([lt, wh], 1).astype(np.int32)

        yuv = torch.randint(0, 256, (8, 1620, 1920), dtype=torch.uint8, device=dev, generator=g)
        rects = yuv_roi_rects(256, 1920, 1080)
        idx = np.arange(256, dtype=np.int32) % 8
        drects, didx = torch.from_numpy(rects).to(dev), torch.from_numpy(idx).to(dev)
        o = torch.empty((256, 112, 112, 3), dtype=torch.uint8, device=dev)
        cases["yuv_crop_resize_rois_1080p_256x112_u8"] = (
            lambda yuv=yuv, drects=drects, didx=didx, o=o: ops.cvt_color_crop_resize_rois(yuv, drects, 112, 112,
                                                                                         src_index=didx, out=o),
            yuv_crop_resize_rois_bytes(112, 112, rects, 1, 1920, 1080), 256 * 112 * 112)
        crop_chains["yuv_crop_resize_rois_1080p_256x112_u8"] = dict(yuv=yuv, rects=drects, idx=didx,
                                                                    out=torch.empty_like(o), norm=False)
        of = torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev)
        cases["yuv_crop_resize_rois_normalize_1080p_256x112_chw"] = (
            lambda yuv=yuv, drects=drects, didx=didx, of=of: ops.cvt_color_crop_resize_rois_normalize(
                yuv, drects, 112, 112, MEAN, STD, src_index=didx, layout=vacv_amd.NCHW, out=of),
            yuv_crop_resize_rois_bytes(112, 112, rects, 4, 1920, 1080), 256 * 112 * 112)
        crop_chains["yuv_crop_resize_rois_normalize_1080p_256x112_chw"] = dict(yuv=yuv, rects=drects, idx=didx,
                                                                               out=torch.empty_like(of), norm=True)
        # the reference harness's crop size: 64 crops of one 1280 x 720 frame
        yuv7 = torch.randint(0, 256, (1, 1080, 1280), dtype=torch.uint8, device=dev, generator=g)
        rects7 = yuv_roi_rects(64, 1280, 720)
        drects7 = torch.from_numpy(rects7).to(dev)
        o7 = torch.empty((64, 210, 140, 3), dtype=torch.uint8, device=dev)
        cases["yuv_crop_resize_rois_720p_64x140x210_u8"] = (
            lambda yuv7=yuv7, drects7=drects7, o7=o7: ops.cvt_color_crop_resize_rois(yuv7, drects7, 140, 210, out=o7),
            yuv_crop_resize_rois_bytes(140, 210, rects7, 1, 1280, 720), 64 * 140 * 210)
        crop_chains["yuv_crop_resize_rois_720p_64x140x210_u8"] = dict(yuv=yuv7, rects=drects7, idx=None,
                                                                      out=torch.empty_like(o7), norm=False)
        # the same boxes, each crop standardized by its own statistics
        # (vacv_cvt_color_crop_resize_rois_standardize); the comparator is the
        # chain it replaces: cvt_color of all frames, then the BGR standardize
        # call, into preallocated buffers
        from vacv_amd.roofline import yuv_crop_resize_rois_standardize_bytes
        os_ = torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev)
        bgr, oc = torch.empty((8, 1080, 1920, 3), dtype=torch.uint8, device=dev), torch.empty_like(os_)

        def crop_std_chain(yuv=yuv, drects=drects, didx=didx, bgr=bgr, oc=oc):
            ops.cvt_color(yuv, out=bgr)
            ops.crop_resize_rois_standardize(bgr, drects, 112, 112, src_index=didx, layout=vacv_amd.NCHW, out=oc)

        cases["yuv_crop_resize_rois_standardize_1080p_256x112_chw"] = (
            lambda yuv=yuv, drects=drects, didx=didx, os_=os_: ops.cvt_color_crop_resize_rois_standardize(
                yuv, drects, 112, 112, src_index=didx, layout=vacv_amd.NCHW, out=os_),
            yuv_crop_resize_rois_standardize_bytes(112, 112, rects, False, 1920, 1080), 256 * 112 * 112)
        std_chains["yuv_crop_resize_rois_standardize_1080p_256x112_chw"] = dict(frames=8, out=oc, chain=crop_std_chain)
    match_loops = {}
    if a.op in ("match_rois", "all"):
        # a tracker's step (vacv_match_template_rois): 256 objects on 8 frames,
        # each its own 32 x 32 template in a 64 x 64 search window around a
        # seeded centre, CCOEFF_NORMED, the peaks included
        import numpy as np
        from vacv_amd.roofline import match_template_rois_bytes
        rng = np.random.default_rng(20261021)
        src = frames(8, 1080, 1920)
        tpls = frames(256, 32, 32)
        centers = torch.from_numpy((rng.random((256, 2)) * [1920, 1080]).astype(np.float32)).to(dev)
        dorg = ops.search_origins(centers, 64, 64, 1920, 1080)
        idx = np.arange(256, dtype=np.int32) % 8
        didx = torch.from_numpy(idx).to(dev)
        o = torch.empty((256, 33, 33), dtype=torch.float32, device=dev)
        method = vacv_amd._lib.TM_CCOEFF_NORMED
        cases["match_rois_1080p_256x64x64_t32_ccoeff_normed"] = (
            lambda src=src, tpls=tpls, dorg=dorg, didx=didx, o=o: ops.match_template_rois(
                src, tpls, dorg, 64, 64, method, src_index=didx, out=o),
            match_template_rois_bytes(3, 64, 64, 32, 32, dorg.cpu().numpy(), 256, True, 1920, 1080), 256 * 33 * 33)
        match_loops["match_rois_1080p_256x64x64_t32_ccoeff_normed"] = dict(
            src=src, tpls=tpls, origins=dorg.cpu().numpy(), idx=idx, w=64, h=64, method=method)
    match_chains = {}
    if a.op in ("yuv_match_rois", "all"):
        # the same step straight from NV21 frames (vacv_cvt_color_match_template_rois)
        import numpy as np
        from vacv_amd.roofline import cvt_color_match_template_rois_bytes
        rng = np.random.default_rng(20261021)
        yuv = torch.randint(0, 256, (8, 1620, 1920), dtype=torch.uint8, device=dev, generator=g)
        tpls = frames(256, 32, 32)
        centers = torch.from_numpy((rng.random((256, 2)) * [1920, 1080]).astype(np.float32)).to(dev)
        dorg = ops.search_origins(centers, 64, 64, 1920, 1080)
        didx = torch.from_numpy(np.arange(256, dtype=np.int32) % 8).to(dev)
        o = torch.empty((256, 33, 33), dtype=torch.float32, device=dev)
        method = vacv_amd._lib.TM_CCOEFF_NORMED
        cases["yuv_match_rois_1080p_256x64x64_t32_ccoeff_normed"] = (
            lambda yuv=yuv, tpls=tpls, dorg=dorg, didx=didx, o=o: ops.cvt_color_match_template_rois(
                yuv, tpls, dorg, 64, 64, method, src_index=didx, out=o),
            cvt_color_match_template_rois_bytes(64, 64, 32, 32, dorg.cpu().numpy(), 256, True, 1920, 1080),
            256 * 33 * 33)
        match_chains["yuv_match_rois_1080p_256x64x64_t32_ccoeff_normed"] = dict(
            yuv=yuv, tpls=tpls, origins=dorg, idx=didx, w=64, h=64, method=method)
    persp_pairs = {}
    if a.op in ("warp_persp_rois", "all"):
        # many small projective crops in ONE launch (vacv_warp_perspective_rois):
        # the warp_rois geometry -- boxes rotated by +-30 degrees, ~250 px per
        # side, centres anywhere in the frame -- with every corner moved by up to
        # 15 % of the side.  The yardstick is vacv_warp_affine_rois[_normalize]
        # on the same boxes without the corner jitter: the neighbouring kernel,
        # the same sampling with cheaper coordinates (orientation only).
        import numpy as np
        rng = np.random.default_rng(20261021)

        def boxes(n, fw, fh, wo, ho, foot=250.0):
            quads, ms = np.zeros((n, 4, 2), np.float32), np.zeros((n, 6), np.float32)
            for i in range(n):
                ang, s = np.deg2rad(rng.uniform(-30.0, 30.0)), max(wo, ho) / foot
                cx, cy = rng.uniform(0, fw), rng.uniform(0, fh)
                ca, sa = np.cos(ang) / s, np.sin(ang) / s  # dst -> src: rotate, scale, centre on (cx, cy)
                inv = np.array([[ca, -sa, cx - ca * wo / 2 + sa * ho / 2], [sa, ca, cy - sa * wo / 2 - ca * ho / 2]])
                ms[i] = inv.reshape(6)
                corners = np.array([[0, 0, 1], [wo - 1, 0, 1], [wo - 1, ho - 1, 1], [0, ho - 1, 1]], np.float64)
                quads[i] = corners @ inv.T + rng.uniform(-0.15, 0.15, (4, 2)) * foot
            return quads, ms

        inv_flag = vacv_amd.INTER_LINEAR | vacv_amd.WARP_INVERSE_MAP
        src = frames(8, 1080, 1920)
        quads, ms = boxes(256, 1920, 1080, 112, 112)
        dhs = ops.homographies_from_quads(torch.from_numpy(quads).to(dev), 112, 112)
        dms = torch.from_numpy(ms).to(dev)
        didx = torch.from_numpy(np.arange(256, dtype=np.int32) % 8).to(dev)
        o, oa = (torch.empty((256, 112, 112, 3), dtype=torch.uint8, device=dev) for _ in range(2))
        nb = 256 * 112 * 112 * 3 * 2  # output bytes + as many source bytes (a crop's footprint is ~5x its pixels; cached)
        cases["warp_persp_rois_1080p_256x112_u8"] = (
            lambda: ops.warp_perspective_rois(src, dhs, 112, 112, src_index=didx, flags=inv_flag, out=o), nb, 256 * 112 * 112)
        persp_pairs["warp_persp_rois_1080p_256x112_u8"] = (
            lambda: ops.warp_affine_rois(src, dms, 112, 112, src_index=didx, flags=inv_flag, out=oa))
        of, ofa = (torch.empty((256, 3, 112, 112), dtype=torch.float32, device=dev) for _ in range(2))
        cases["warp_persp_rois_normalize_1080p_256x112_chw"] = (
            lambda: ops.warp_perspective_rois_normalize(src, dhs, 112, 112, MEAN, STD, src_index=didx,
                                                        out_layout=vacv_amd.NCHW, flags=inv_flag, out=of),
            256 * 112 * 112 * 3 * 5, 256 * 112 * 112)
        persp_pairs["warp_persp_rois_normalize_1080p_256x112_chw"] = (
            lambda: ops.warp_affine_rois_normalize(src, dms, 112, 112, MEAN, STD, src_index=didx,
                                                   out_layout=vacv_amd.NCHW, flags=inv_flag, out=ofa))
        src7 = frames(1, 720, 1280)
        quads7, ms7 = boxes(64, 1280, 720, 140, 210)
        dhs7 = ops.homographies_from_quads(torch.from_numpy(quads7).to(dev), 140, 210)
        dms7 = torch.from_numpy(ms7).to(dev)
        o7, o7a = (torch.empty((64, 210, 140, 3), dtype=torch.uint8, device=dev) for _ in range(2))
        cases["warp_persp_rois_720p_64x140x210_u8"] = (
            lambda: ops.warp_perspective_rois(src7, dhs7, 140, 210, flags=inv_flag, out=o7), 64 * 140 * 210 * 3 * 2,
            64 * 140 * 210)
        persp_pairs["warp_persp_rois_720p_64x140x210_u8"] = (
            lambda: ops.warp_affine_rois(src7, dms7, 140, 210, flags=inv_flag, out=o7a))
    if a.only:
        cases = {k: v for k, v in cases.items() if a.only in k}
    if a.compare and a.op == "warp_persp_rois":
        compare_persp_with_affine({k: v for k, v in cases.items() if k in persp_pairs}, persp_pairs, a.iters)
        return
    if a.compare and a.op == "yuv_match_rois":
        compare_with_match_chains({k: v for k, v in cases.items() if k in match_chains}, match_chains, a.iters)
        return
    if a.compare and a.op == "match_rois":
        compare_with_match_loops({k: v for k, v in cases.items() if k in match_loops}, match_loops, a.iters)
        return
    if a.compare and a.op == "yuv_crop_resize_rois":
        compare_with_crop_chains({k: v for k, v in cases.items() if k in crop_chains}, crop_chains, a.baseline_lib,
                                 a.iters)
        compare_with_std_chains({k: v for k, v in cases.items() if k in std_chains}, std_chains, a.iters)
        return
    if a.compare and a.op == "crop_resize_rois":
        compare_with_crop_loops({k: v for k, v in cases.items() if k in crop_loops}, crop_loops, a.iters)
        compare_with_std_chains({k: v for k, v in cases.items() if k in std_chains}, std_chains, a.iters)
        return
    if a.compare and a.op == "yuv_rois":
        compare_with_chains({k: v for k, v in cases.items() if k in chains}, chains, a.baseline_lib, a.iters)
        compare_with_std_chains({k: v for k, v in cases.items() if k in std_chains}, std_chains, a.iters)
        return
    if a.compare:
        compare_with_loops({k: v for k, v in cases.items() if k in loops}, loops, a.baseline_lib, a.iters)
        compare_with_std_chains({k: v for k, v in cases.items() if k in std_chains}, std_chains, a.iters)
        return
    import itertools
    knobs = [kv.split("=", 1) for kv in a.sweep.split(";") if kv]
    combos = list(itertools.product(*[[(k, v) for v in vals.split(",")] for k, vals in knobs])) or [()]
    for fn, _, _ in cases.values():  # clocks ramp before the first timed case
        for _ in range(100):
            fn()
    torch.cuda.synchronize()
    for combo in combos:
        for k, v in combo:
            ops.set_tuning(k, int(v))
        tag = " ".join(f"{k}={v}" for k, v in combo)
        run_cases(cases, a.iters, tag)


def compare_persp_with_affine(cases, pairs, iters):
    """--op warp_persp_rois: vacv_warp_perspective_rois[_normalize] against
    vacv_warp_affine_rois[_normalize] on the same boxes without the corner
    jitter, on this build: alternating, medians, end to end (host clock around
    a synchronised stream) and between HIP events.  The affine call computes
    OTHER crops (no projective part): the ratio says what the fp64 coordinates
    cost next to the float ones, nothing about correctness."""
    import time

    import torch

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def event_ms(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s = torch.cuda.current_stream()
        e0.record(s)
        f()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def med(v):
        return sorted(v)[len(v) // 2]

    for name, (fn, nbytes, px) in cases.items():
        aff = pairs[name]
        for _ in range(100):  # clocks ramp before the first timed call
            aff()
            fn()
        torch.cuda.synchronize()
        t_p, t_a, e_p, e_a = [], [], [], []
        for _ in range(iters):
            t_a.append(timed(aff))
            t_p.append(timed(fn))
            e_a.append(event_ms(aff))
            e_p.append(event_ms(fn))
        print(json.dumps({"case": name, "pixels": int(px), "iters": iters,
                          "persp_ms_median": round(med(t_p), 4), "persp_ms_min": round(min(t_p), 4),
                          "affine_ms_median": round(med(t_a), 4), "affine_ms_min": round(min(t_a), 4),
                          "persp_over_affine": round(med(t_p) / med(t_a), 3),
                          "persp_events_ms_median": round(med(e_p), 4), "affine_events_ms_median": round(med(e_a), 4),
                          "persp_over_affine_events": round(med(e_p) / med(e_a), 3),
                          "persp_Gpx_per_s_events": round(px / med(e_p) / 1e6, 2),
                          "clock": "host, stream synchronised; HIP events on the stream"}), flush=True)


def compare_with_loops(cases, loops, baseline_lib, iters):
    """One call for all crops against a loop of single calls, per case: both
    timed end to end with a host clock around a synchronised stream (the
    loop's time is mostly launches and host plans, which device events would
    not see), alternating, after warm-up.  The loop's descriptors, matrices and
    ctypes references are built beforehand, so what is timed is the library."""
    import ctypes
    import time

    import torch
    import vacv_amd
    from vacv_amd import _lib as L, ops
    if baseline_lib:
        # another build by its own handle: only entry points both builds share
        base = ctypes.CDLL(str(Path(baseline_lib).resolve()))
        for fname in ("vacv_warp_affine", "vacv_warp_affine_normalize", "vacv_change_layout", "vacv_abi_version"):
            getattr(base, fname).argtypes, getattr(base, fname).restype = L.SIGNATURES[fname]
        tag = f"{baseline_lib} (ABI {base.vacv_abi_version()})"
    else:
        base, tag = L.load(), "this build"
    stream = ops._stream()
    bv = (ctypes.c_double * 4)(0, 0, 0, 0)
    mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    for name, (fn, nbytes, px) in cases.items():
        lp = loops[name]
        src, ms, idx, out, norm = lp["src"], lp["ms"], lp["idx"], lp["out"], lp["norm"]
        n = len(ms)
        ho, wo = (out.shape[2], out.shape[3]) if norm else (out.shape[1], out.shape[2])
        tmp = torch.empty((n, ho, wo, 3), dtype=torch.float32, device=out.device) if norm else out
        keep = [ops.describe(src[i:i + 1]) for i in range(src.shape[0])] + [ops.describe(tmp[i:i + 1]) for i in range(n)]
        fd = [ctypes.byref(d) for d in keep[:src.shape[0]]]
        dd = [ctypes.byref(d) for d in keep[src.shape[0]:]]
        mp = [(ctypes.c_float * 6)(*[float(v) for v in m]) for m in ms]
        whole_tmp, whole_out = ops.describe(tmp), ops.describe(out, vacv_amd.NCHW if norm else vacv_amd.NHWC)
        frame_of = [int(k) for k in idx]

        def loop():
            if norm:
                for i in range(n):
                    assert base.vacv_warp_affine_normalize(fd[frame_of[i]], dd[i], mp[i], 1, 0, bv, mean, std, stream) == 0
                assert base.vacv_change_layout(ctypes.byref(whole_tmp), ctypes.byref(whole_out), stream) == 0
            else:
                for i in range(n):
                    assert base.vacv_warp_affine(fd[frame_of[i]], dd[i], mp[i], 1, 0, bv, stream) == 0

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(5):
            loop()
            one = fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(one, out))  # both legs compute the same crops
        t_loop, t_one = [], []
        for _ in range(iters):
            t_loop.append(timed(loop))
            t_one.append(timed(fn))
        ml, mo = sorted(t_loop)[iters // 2], sorted(t_one)[iters // 2]
        print(json.dumps({"case": name, "rois": n, "baseline": tag, "loop_ms_median": round(ml, 4),
                          "loop_ms_min": round(min(t_loop), 4), "one_call_ms_median": round(mo, 4),
                          "one_call_ms_min": round(min(t_one), 4), "loop_over_one_call": round(ml / mo, 2),
                          "alg_bytes": int(nbytes), "one_call_alg_GBps": round(nbytes / mo / 1e6, 1),
                          "outputs_equal": same, "clock": "host, stream synchronised"}), flush=True)


def compare_with_chains(cases, chains, baseline_lib, iters):
    """--op yuv_rois: the one call against the chain it replaces -- vacv_cvt_color
    of all frames into a BGR buffer, then vacv_warp_affine_rois[_normalize] on
    it -- per case, both timed end to end with a host clock around a
    synchronised stream, alternating, after warm-up; outputs compared equal.
    The chain runs on `baseline_lib` (e.g. the parent commit's build) by its
    own handle, or on this build.  Descriptors and ctypes references are built
    beforehand for both legs, so what is timed is the library (the binding's
    own argument handling is tens of microseconds, as much as either leg)."""
    import ctypes
    import time

    import torch
    import vacv_amd
    from vacv_amd import _lib as L, ops
    lib = L.load()
    if baseline_lib:
        base = ctypes.CDLL(str(Path(baseline_lib).resolve()))
        for fname in ("vacv_cvt_color", "vacv_warp_affine_rois", "vacv_warp_affine_rois_normalize", "vacv_abi_version"):
            getattr(base, fname).argtypes, getattr(base, fname).restype = L.SIGNATURES[fname]
        tag = f"{baseline_lib} (ABI {base.vacv_abi_version()})"
    else:
        base, tag = lib, "this build"
    stream = ops._stream()
    bv = (ctypes.c_double * 4)(0, 0, 0, 0)
    mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    for name, (binding_call, nbytes, px) in cases.items():
        ch = chains[name]
        yuv, ms, idx, out, norm = ch["yuv"], ch["ms"], ch["idx"], ch["out"], ch["norm"]
        bgr = torch.empty((yuv.shape[0], yuv.shape[1] // 3 * 2, yuv.shape[2], 3), dtype=torch.uint8, device=yuv.device)
        yd, bd = ops._yuv_desc(yuv), ops.describe(bgr)
        od = ops.describe(out, vacv_amd.NCHW if norm else vacv_amd.NHWC)
        mp, ip = ms.data_ptr(), (idx.data_ptr() if idx is not None else None)

        def chain():
            assert base.vacv_cvt_color(ctypes.byref(yd), ctypes.byref(bd), L.COLOR_YUV2BGR_NV21, stream) == 0
            if norm:
                assert base.vacv_warp_affine_rois_normalize(ctypes.byref(bd), ctypes.byref(od), mp, ip, 1, 0, bv, mean, std,
                                                            stream) == 0
            else:
                assert base.vacv_warp_affine_rois(ctypes.byref(bd), ctypes.byref(od), mp, ip, 1, 0, bv, stream) == 0

        one = binding_call()  # the binding's own output tensor, written by the calls below
        od1 = ops.describe(one, vacv_amd.NCHW if norm else vacv_amd.NHWC)

        def fn():
            if norm:
                assert lib.vacv_cvt_color_warp_affine_rois_normalize(ctypes.byref(yd), ctypes.byref(od1),
                                                                     L.COLOR_YUV2BGR_NV21, mp, ip, 1, 0, bv, mean, std,
                                                                     stream) == 0
            else:
                assert lib.vacv_cvt_color_warp_affine_rois(ctypes.byref(yd), ctypes.byref(od1), L.COLOR_YUV2BGR_NV21, mp,
                                                           ip, 1, 0, bv, stream) == 0

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        one.zero_()
        for _ in range(20):
            chain()
            fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(one, out))  # both legs compute the same crops
        t_chain, t_one = [], []
        for _ in range(iters):
            t_chain.append(timed(chain))
            t_one.append(timed(fn))
        t_chain.sort()
        t_one.sort()
        mc, mo = t_chain[iters // 2], t_one[iters // 2]
        print(json.dumps({"case": name, "rois": int(ms.shape[0]), "frames": int(yuv.shape[0]), "baseline": tag,
                          "chain_ms_median": round(mc, 4), "chain_ms_min": round(t_chain[0], 4),
                          "chain_ms_p10": round(t_chain[iters // 10], 4), "chain_ms_p90": round(t_chain[iters * 9 // 10], 4),
                          "one_call_ms_median": round(mo, 4), "one_call_ms_min": round(t_one[0], 4),
                          "one_call_ms_p90": round(t_one[iters * 9 // 10], 4),
                          "chain_over_one_call": round(mc / mo, 2), "alg_bytes": int(nbytes),
                          "one_call_alg_GBps": round(nbytes / mo / 1e6, 1), "outputs_equal": same,
                          "clock": "host, stream synchronised"}), flush=True)


def compare_with_crop_chains(cases, chains, baseline_lib, iters):
    """--op yuv_crop_resize_rois: the one call against the chain it replaces --
    vacv_cvt_color of all frames into a preallocated BGR buffer, then
    vacv_crop_resize_rois[_normalize] on it -- per case, both timed end to end
    with a host clock around a synchronised stream, alternating, after warm-up;
    medians with p10-p90, outputs compared equal.  The chain runs on
    `baseline_lib` (e.g. the parent commit's build) by its own handle, or on
    this build.  Both legs are ctypes calls whose descriptors were built
    beforehand, so what is timed is the library."""
    import ctypes
    import time

    import torch
    import vacv_amd
    from vacv_amd import _lib as L, ops
    lib = L.load()
    if baseline_lib:
        base = ctypes.CDLL(str(Path(baseline_lib).resolve()))
        for fname in ("vacv_cvt_color", "vacv_crop_resize_rois", "vacv_crop_resize_rois_normalize", "vacv_abi_version"):
            getattr(base, fname).argtypes, getattr(base, fname).restype = L.SIGNATURES[fname]
        tag = f"{baseline_lib} (ABI {base.vacv_abi_version()})"
    else:
        base, tag = lib, "this build"
    stream = ops._stream()
    mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    code, linear, ref = L.COLOR_YUV2BGR_NV21, vacv_amd.INTER_LINEAR, vacv_amd.LINEAR_REFERENCE
    for name, (binding_call, nbytes, px) in cases.items():
        ch = chains[name]
        yuv, rects, idx, out, norm = ch["yuv"], ch["rects"], ch["idx"], ch["out"], ch["norm"]
        bgr = torch.empty((yuv.shape[0], yuv.shape[1] // 3 * 2, yuv.shape[2], 3), dtype=torch.uint8, device=yuv.device)
        yd, bd = ops._yuv_desc(yuv), ops.describe(bgr)
        od = ops.describe(out, vacv_amd.NCHW if norm else vacv_amd.NHWC)
        rp, ip = rects.data_ptr(), (idx.data_ptr() if idx is not None else None)

        def chain():
            assert base.vacv_cvt_color(ctypes.byref(yd), ctypes.byref(bd), code, stream) == 0
            if norm:
                assert base.vacv_crop_resize_rois_normalize(ctypes.byref(bd), ctypes.byref(od), rp, ip, linear, ref, mean,
                                                            std, stream) == 0
            else:
                assert base.vacv_crop_resize_rois(ctypes.byref(bd), ctypes.byref(od), rp, ip, linear, ref, stream) == 0

        one = binding_call()  # the binding's own output tensor, written by the calls below
        od1 = ops.describe(one, vacv_amd.NCHW if norm else vacv_amd.NHWC)

        def fn():
            if norm:
                assert lib.vacv_cvt_color_crop_resize_rois_normalize(ctypes.byref(yd), ctypes.byref(od1), code, rp, ip,
                                                                     linear, ref, mean, std, stream) == 0
            else:
                assert lib.vacv_cvt_color_crop_resize_rois(ctypes.byref(yd), ctypes.byref(od1), code, rp, ip, linear, ref,
                                                           stream) == 0

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        one.zero_()
        for _ in range(20):
            chain()
            fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(one, out))  # both legs compute the same crops
        t_chain, t_one = [], []
        for _ in range(iters):
            t_chain.append(timed(chain))
            t_one.append(timed(fn))
        t_chain.sort()
        t_one.sort()
        mc, mo = t_chain[iters // 2], t_one[iters // 2]
        c10, c90 = t_chain[iters // 10], t_chain[iters * 9 // 10]
        print(json.dumps({"case": name, "rois": int(rects.shape[0]), "frames": int(yuv.shape[0]), "baseline": tag,
                          "iters": iters, "chain_ms_median": round(mc, 4), "chain_ms_min": round(t_chain[0], 4),
                          "chain_ms_p10": round(c10, 4), "chain_ms_p90": round(c90, 4),
                          "chain_p10_p90_half_width_ms": round((c90 - c10) / 2, 4),
                          "one_call_ms_median": round(mo, 4), "one_call_ms_min": round(t_one[0], 4),
                          "one_call_ms_p10": round(t_one[iters // 10], 4),
                          "one_call_ms_p90": round(t_one[iters * 9 // 10], 4),
                          "chain_over_one_call": round(mc / mo, 2),
                          "one_call_within_chain_noise": bool(mo <= mc + (c90 - c10) / 2), "alg_bytes": int(nbytes),
                          "one_call_alg_GBps": round(nbytes / mo / 1e6, 1), "outputs_equal": same,
                          "clock": "host, stream synchronised"}), flush=True)


def compare_with_crop_loops(cases, loops, iters):
    """--op crop_resize_rois: the one call against the same crops as a loop of
    vacv_crop + vacv_resize (or vacv_resize_normalize, then one
    vacv_change_layout) single calls on this build, per case: both timed end to
    end with a host clock around a synchronised stream, alternating, after
    warm-up; outputs compared equal.  The loop's descriptors, crop buffers and
    ctypes references are built beforehand, so what is timed is the library.
    Also per case the one call's time between device events (the kernel), and
    for the 112 x 112 cases that of vacv_warp_affine_rois[_normalize] on the
    scale-and-translate maps of the same boxes (the neighbouring kernel doing
    comparable work, other arithmetic: for orientation only)."""
    import ctypes
    import time

    import numpy as np
    import torch
    import vacv_amd
    from vacv_amd import _lib as L, ops
    lib = L.load()
    stream = ops._stream()
    mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)

    def events_ms(f):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        s = torch.cuda.current_stream()
        for e0, e1 in ev:
            e0.record(s)
            f()
            e1.record(s)
        torch.cuda.synchronize()
        return sorted(e0.elapsed_time(e1) for e0, e1 in ev)[iters // 2]

    for name, (fn, nbytes, px) in cases.items():
        lp = loops[name]
        src, rects, idx, out, norm = lp["src"], lp["rects"], lp["idx"], lp["out"], lp["norm"]
        n = len(rects)
        ho, wo = (out.shape[2], out.shape[3]) if norm else (out.shape[1], out.shape[2])
        tmp = torch.empty((n, ho, wo, 3), dtype=torch.float32, device=out.device) if norm else out
        crops = [torch.empty((1, int(h), int(w), 3), dtype=torch.uint8, device=out.device) for _, _, w, h in rects]
        keep = ([ops.describe(src[i:i + 1]) for i in range(src.shape[0])], [ops.describe(c) for c in crops],
                [ops.describe(tmp[i:i + 1]) for i in range(n)])
        fd, cd, dd = ([ctypes.byref(d) for d in ds] for ds in keep)
        whole_tmp, whole_out = ops.describe(tmp), ops.describe(out, vacv_amd.NCHW if norm else vacv_amd.NHWC)
        frame_of = [int(k) for k in idx]
        lt = [(int(r[0]), int(r[1])) for r in rects]

        def loop():
            for i in range(n):
                assert lib.vacv_crop(fd[frame_of[i]], cd[i], lt[i][0], lt[i][1], stream) == 0
                if norm:
                    assert lib.vacv_resize_normalize(cd[i], dd[i], 1, 0, mean, std, stream) == 0
                else:
                    assert lib.vacv_resize(cd[i], dd[i], 1, 0, stream) == 0
            if norm:
                assert lib.vacv_change_layout(ctypes.byref(whole_tmp), ctypes.byref(whole_out), stream) == 0

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(5):
            loop()
            one = fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(one, out))  # both legs compute the same crops
        t_loop, t_one = [], []
        for _ in range(iters):
            t_loop.append(timed(loop))
            t_one.append(timed(fn))
        ml, mo = sorted(t_loop)[iters // 2], sorted(t_one)[iters // 2]
        line = {"case": name, "rois": n, "frames": int(src.shape[0]), "baseline": "this build",
                "loop_ms_median": round(ml, 4), "loop_ms_min": round(min(t_loop), 4),
                "one_call_ms_median": round(mo, 4), "one_call_ms_min": round(min(t_one), 4),
                "loop_over_one_call": round(ml / mo, 2), "kernel_ms_median": round(events_ms(fn), 4),
                "alg_bytes": int(nbytes), "outputs_equal": same, "clock": "host, stream synchronised; kernel: events"}
        if (wo, ho) == (112, 112):
            # dst = s * src + t with the box onto the whole output
            sx, sy = wo / rects[:, 2].astype(np.float64), ho / rects[:, 3].astype(np.float64)
            ms = np.stack([sx, 0 * sx, -sx * rects[:, 0], 0 * sy, sy, -sy * rects[:, 1]], 1).astype(np.float32)
            dms, didx = torch.from_numpy(ms).to(out.device), torch.from_numpy(np.asarray(idx, np.int32)).to(out.device)
            wout = torch.empty_like(out)
            if norm:
                warp = lambda: ops.warp_affine_rois_normalize(src, dms, wo, ho, MEAN, STD, src_index=didx,
                                                              out_layout=vacv_amd.NCHW, out=wout)
            else:
                warp = lambda: ops.warp_affine_rois(src, dms, wo, ho, src_index=didx, out=wout)
            for _ in range(5):
                warp()
            torch.cuda.synchronize()
            line["warp_rois_same_boxes_kernel_ms_median"] = round(events_ms(warp), 4)
        print(json.dumps(line), flush=True)


def compare_with_std_chains(cases, chains, iters):
    """--op crop_resize_rois and --op warp_rois, the standardize cases: the one
    call against the chain it replaces on this build (--op yuv_rois and --op
    yuv_crop_resize_rois: ops.cvt_color of all frames, then the BGR standardize
    call, the case's own "chain") -- ops.crop_resize_rois or
    ops.warp_affine_rois (the chain's "u8" stage) into a u8 batch,
    ops.normalize(None, None) (the per-image statistics and the normalize) into
    an fp32 NHWC batch, ops.change_layout into the NCHW output, every buffer
    preallocated -- both timed end to end with a host clock around a
    synchronised stream, alternating, after warm-up; medians with p10-p90,
    outputs compared equal.  Also the one call's time between device events
    (the kernel)."""
    import time

    import torch
    import vacv_amd
    from vacv_amd import ops

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, (fn, nbytes, px) in cases.items():
        ch = chains[name]
        out = ch["out"]
        n, c, ho, wo = out.shape
        if "chain" in ch:  # the YUV cases: cvt_color + the BGR standardize call, writing `out`
            chain = ch["chain"]
        else:
            first = ch["u8"]
            u = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=out.device)
            f32 = torch.empty((n, ho, wo, c), dtype=torch.float32, device=out.device)

            def chain(first=first, u=u, f32=f32, out=out):
                first(u)
                ops.normalize(u, None, None, out=f32)
                ops.change_layout(f32, vacv_amd.NCHW, out=out)

        for _ in range(20):
            chain()
            one = fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(one.view(torch.int32), out.view(torch.int32)))  # bit for bit
        t_chain, t_one = [], []
        for _ in range(iters):
            t_chain.append(timed(chain))
            t_one.append(timed(fn))
        t_chain.sort()
        t_one.sort()
        mc, mo = t_chain[iters // 2], t_one[iters // 2]
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        s = torch.cuda.current_stream()
        for e0, e1 in ev:
            e0.record(s)
            fn()
            e1.record(s)
        torch.cuda.synchronize()
        kernel = sorted(e0.elapsed_time(e1) for e0, e1 in ev)[iters // 2]
        evc = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for e0, e1 in evc:
            e0.record(s)
            chain()
            e1.record(s)
        torch.cuda.synchronize()
        chain_ev = sorted(e0.elapsed_time(e1) for e0, e1 in evc)[iters // 2]
        print(json.dumps({"case": name, "rois": int(n), "frames": int(ch["frames"]), "baseline": "this build",
                          "iters": iters, "chain_ms_median": round(mc, 4), "chain_ms_min": round(t_chain[0], 4),
                          "chain_ms_p10": round(t_chain[iters // 10], 4), "chain_ms_p90": round(t_chain[iters * 9 // 10], 4),
                          "one_call_ms_median": round(mo, 4), "one_call_ms_min": round(t_one[0], 4),
                          "one_call_ms_p10": round(t_one[iters // 10], 4),
                          "one_call_ms_p90": round(t_one[iters * 9 // 10], 4),
                          "chain_over_one_call": round(mc / mo, 2), "kernel_ms_median": round(kernel, 4),
                          "chain_events_ms_median": round(chain_ev, 4), "alg_bytes": int(nbytes),
                          "kernel_alg_GBps": round(nbytes / kernel / 1e6, 1), "outputs_equal": same,
                          "clock": "host, stream synchronised; kernel and chain_events: device events"}), flush=True)


def compare_with_match_loops(cases, loops, iters):
    """--op match_rois: the one call against the same work as the loop it
    replaces -- vacv_crop + vacv_match_template + vacv_min_max_idx per ROI on
    this build (about 8 launches each) -- per case: both timed end to end with
    a host clock around a synchronised stream, alternating, after warm-up; maps
    and peaks compared equal.  The loop's descriptors, crop buffers and ctypes
    references are built beforehand, so what is timed is the library.  Also the
    one call's time between device events (the kernel)."""
    import ctypes
    import time

    import torch
    from vacv_amd import _lib as L, ops
    lib = L.load()
    stream = ops._stream()

    for name, (fn, nbytes, px) in cases.items():
        lp = loops[name]
        src, tpls, origins, idx, w, h, method = (lp[k] for k in ("src", "tpls", "origins", "idx", "w", "h", "method"))
        n, c = len(origins), src.shape[3]
        rh, rw = h - tpls.shape[1] + 1, w - tpls.shape[2] + 1
        dev = src.device
        crops = torch.empty((n, h, w, c), dtype=torch.uint8, device=dev)
        maps = torch.empty((n, rh, rw, 1), dtype=torch.float32, device=dev)
        vals = torch.empty((n, 2), dtype=torch.float64, device=dev)
        peaks = torch.empty((n, 4), dtype=torch.int32, device=dev)
        keep = ([ops.describe(src[i:i + 1]) for i in range(src.shape[0])], [ops.describe(crops[i:i + 1]) for i in range(n)],
                [ops.describe(tpls[i:i + 1]) for i in range(n)], [ops.describe(maps[i:i + 1]) for i in range(n)],
                [ops.describe(maps[i, :, :, 0]) for i in range(n)])
        fd, cd, td, md, m2 = ([ctypes.byref(d) for d in ds] for ds in keep)
        vp = [vals[i].data_ptr() for i in range(n)]
        ip = [peaks[i].data_ptr() for i in range(n)]
        frame_of = [int(k) for k in idx]
        lt = [(int(o[0]), int(o[1])) for o in origins]

        def loop():
            for i in range(n):
                assert lib.vacv_crop(fd[frame_of[i]], cd[i], lt[i][0], lt[i][1], stream) == 0
                assert lib.vacv_match_template(cd[i], td[i], md[i], method, stream) == 0
                assert lib.vacv_min_max_idx(m2[i], None, vp[i], ip[i], stream) == 0

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(5):
            loop()
            one = fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(one[0], maps[..., 0]) and torch.equal(one[1], vals) and torch.equal(one[2], peaks))
        t_loop, t_one = [], []
        for _ in range(iters):
            t_loop.append(timed(loop))
            t_one.append(timed(fn))
        ml, mo = sorted(t_loop)[iters // 2], sorted(t_one)[iters // 2]
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        s = torch.cuda.current_stream()
        for e0, e1 in ev:
            e0.record(s)
            fn()
            e1.record(s)
        torch.cuda.synchronize()
        kernel = sorted(e0.elapsed_time(e1) for e0, e1 in ev)[iters // 2]
        print(json.dumps({"case": name, "rois": n, "frames": int(src.shape[0]), "baseline": "this build",
                          "loop_ms_median": round(ml, 4), "loop_ms_min": round(min(t_loop), 4),
                          "one_call_ms_median": round(mo, 4), "one_call_ms_min": round(min(t_one), 4),
                          "loop_over_one_call": round(ml / mo, 2), "kernel_ms_median": round(kernel, 4),
                          "alg_bytes": int(nbytes), "outputs_equal": same,
                          "clock": "host, stream synchronised; kernel: events"}), flush=True)


def compare_with_match_chains(cases, chains, iters):
    """--op yuv_match_rois: the one call against the chain it replaces --
    vacv_cvt_color of all frames into a preallocated BGR buffer, then
    vacv_match_template_rois on it, on this build (no line of either changed
    with the fused call, so they are the parent commit's) -- per case: both
    timed end to end with a host clock around a synchronised stream,
    alternating, after warm-up; medians with p10-p90; maps, vals and idx compared
    equal.  Both legs are ctypes calls whose descriptors were built beforehand,
    so what is timed is the library.  Also between device events (the kernels):
    the one call, vacv_cvt_color alone and vacv_match_template_rois alone."""
    import ctypes
    import time

    import torch
    from vacv_amd import _lib as L, ops
    lib = L.load()
    stream = ops._stream()
    code = L.COLOR_YUV2BGR_NV21
    by = ctypes.byref

    def events_ms(f):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        s = torch.cuda.current_stream()
        for e0, e1 in ev:
            e0.record(s)
            f()
            e1.record(s)
        torch.cuda.synchronize()
        return sorted(e0.elapsed_time(e1) for e0, e1 in ev)[iters // 2]

    for name, (binding_call, nbytes, px) in cases.items():
        ch = chains[name]
        yuv, tpls, origins, idx, w, h, method = (ch[k] for k in ("yuv", "tpls", "origins", "idx", "w", "h", "method"))
        n, dev = origins.shape[0], yuv.device
        rh, rw = h - tpls.shape[1] + 1, w - tpls.shape[2] + 1
        bgr = torch.empty((yuv.shape[0], yuv.shape[1] // 3 * 2, yuv.shape[2], 3), dtype=torch.uint8, device=dev)
        maps = [torch.empty((n, rh, rw, 1), dtype=torch.float32, device=dev) for _ in range(2)]
        vals = [torch.empty((n, 2), dtype=torch.float64, device=dev) for _ in range(2)]
        peaks = [torch.empty((n, 4), dtype=torch.int32, device=dev) for _ in range(2)]
        yd, bd, td = ops._yuv_desc(yuv), ops.describe(bgr), ops.describe(tpls)
        md = [ops.describe(m) for m in maps]
        op_, ip = origins.data_ptr(), idx.data_ptr()
        vp, pp = [v.data_ptr() for v in vals], [p.data_ptr() for p in peaks]

        def decode():
            assert lib.vacv_cvt_color(by(yd), by(bd), code, stream) == 0

        def match():
            assert lib.vacv_match_template_rois(by(bd), by(td), by(md[0]), op_, ip, method, vp[0], pp[0], stream) == 0

        def chain():
            decode()
            match()

        def fn():
            assert lib.vacv_cvt_color_match_template_rois(by(yd), by(td), by(md[1]), code, op_, ip, method, vp[1], pp[1],
                                                          stream) == 0

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        binding_call()  # the binding's own path works on the same operands
        for t in maps + vals + peaks:
            t.zero_()
        for _ in range(20):
            chain()
            fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(maps[0].view(torch.int32), maps[1].view(torch.int32)) and
                    torch.equal(vals[0].view(torch.int64), vals[1].view(torch.int64)) and torch.equal(peaks[0], peaks[1]))
        t_chain, t_one = [], []
        for _ in range(iters):
            t_chain.append(timed(chain))
            t_one.append(timed(fn))
        t_chain.sort()
        t_one.sort()
        mc, mo = t_chain[iters // 2], t_one[iters // 2]
        k_one, k_decode, k_match = events_ms(fn), events_ms(decode), events_ms(match)
        print(json.dumps({"case": name, "rois": int(n), "frames": int(yuv.shape[0]), "baseline": "this build",
                          "iters": iters, "chain_ms_median": round(mc, 4), "chain_ms_min": round(t_chain[0], 4),
                          "chain_ms_p10": round(t_chain[iters // 10], 4), "chain_ms_p90": round(t_chain[iters * 9 // 10], 4),
                          "one_call_ms_median": round(mo, 4), "one_call_ms_min": round(t_one[0], 4),
                          "one_call_ms_p10": round(t_one[iters // 10], 4),
                          "one_call_ms_p90": round(t_one[iters * 9 // 10], 4),
                          "chain_over_one_call": round(mc / mo, 2), "one_call_at_most_chain": bool(mo <= mc),
                          "kernel_ms_median": round(k_one, 4), "cvt_color_kernel_ms_median": round(k_decode, 4),
                          "match_rois_kernel_ms_median": round(k_match, 4),
                          "kernel_at_most_sum": bool(k_one <= k_decode + k_match),
                          "alg_bytes": int(nbytes), "one_call_alg_GBps": round(nbytes / mo / 1e6, 1),
                          "outputs_equal": same,
                          "clock": "host, stream synchronised; kernels: events"}), flush=True)


def run_cases(cases, iters, tag):
    import torch
    for name, (fn, nbytes, px) in cases.items():
        for _ in range(10):  # clocks settle before the timed launches
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        s = torch.cuda.current_stream()
        for e0, e1 in ev:
            e0.record(s)
            fn()
            e1.record(s)
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        med = ms[len(ms) // 2]
        if name.endswith("_macs"):
            # a compute rate, not bytes: u8 multiply-adds of the correlation
            # per second, against the dense i8 MFMA peak (~5 POP/s = 2.5
            # PMAC/s, MI355X_MICROARCH.md; the kernel's nibble split issues
            # twice these MACs on the matrix cores)
            rate = {"GMAC_s": round(nbytes / med / 1e6, 1), "frac_i8_mfma_dense": round(nbytes / med / 1e6 / 2.5e6, 4)}
        else:
            rate = {"alg_GBps": round(nbytes / med / 1e6, 1), "frac_8TBps": round(nbytes / med / 1e6 / 8000, 4)}
        print(json.dumps({"case": name, **({"knobs": tag} if tag else {}), "ms_median": round(med, 4),
                          "ms_min": round(ms[0], 4), **rate, "Mpx_s": round(px / med / 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
