"""What the input entries refuse, entry by entry: the 8-bit, tensor and YUV entries, their resized forms, the three stream_open calls
and the settings in front of them (set_input_resize, set_yuv_layout, yuv_to_rgb8); then the oriented, the oriented resized and the video
entries and their three stream_open calls (FAMILY_ROWS), which are called by their C names so that a row says which entry it enters.

One table.  A row is a bad call, the error code it returns and a piece of the message it leaves: the entry's name and the reason, as
the library words them.  A call that is wrong in two ways names the check that comes first.  Nothing is launched for a refused call;
after every refusal a good call on the same context still succeeds.
"""
import ctypes as C

import pytest

from acf_amd import capi, synth

pytestmark = pytest.mark.gpu

PH, PW = 96, 128          # the plans
SH, SW, SCALE = 192, 256, 0.5   # the unreduced frames of the resized entries
NAN, INF = float("nan"), float("inf")


class Ctxs:
    """The contexts of the table, made once: three-plane, one-plane, five-plane, an odd-sized plan, sub-batch streams, and a three-plane
    one whose plan is the quarter turn of the others' (128 x 96)."""

    def __init__(self):
        import torch
        from acf_amd.detector import HipDetector
        self.torch = torch
        self.D = HipDetector
        self.tiny = synth.make_model(seed=3, name="TINY", nTrees=16)
        self.buf = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")   # room on both sides of `ptr` for every call below, were it not refused
        self.ptr = self.buf.data_ptr() + (1 << 21)
        self.x = self.buf[1 << 21:]
        self.f32 = torch.zeros((2, 5, PW, PH), dtype=torch.float32, device="cuda")
        self.three = HipDetector(self.tiny, PH, PW, 3, max_batch=2)
        self.one = HipDetector(synth.make_model(seed=3, name="FACE64", nTrees=16), PH, PW, 1, max_batch=2)
        self.five = HipDetector(self.tiny, PH, PW, 5, max_batch=2)
        self.odd = HipDetector(self.tiny, PH + 1, PW, 3, max_batch=2)
        self.multi = HipDetector(self.tiny, PH, PW, 3, max_batch=4, streams=2)
        self.turn = HipDetector(self.tiny, PW, PH, 3, max_batch=2)
        self.yuv, self.fb = HipDetector.yuv_desc("i420", PH, PW)
        self.yuvS, self.fbS = HipDetector.yuv_desc("i420", SH, SW)
        self.img = capi.ImageDesc(capi.T_U8, 3, 3 * PH * PW, PH * PW, PW, 1)
        self.imgS = capi.ImageDesc(capi.T_U8, 3, 3 * SH * SW, SH * SW, SW, 1)
        self.f709, self.f10 = capi.YuvFormat(8, 0, capi.YUV_MATRIX_BT709, 0), capi.YuvFormat(10, 6, capi.YUV_MATRIX_BT2020, 0)
        self.yuv10, self.fb10 = HipDetector.video_desc("nv12", PH, PW, self.f10)

    def bare(self):
        return self.D(self.tiny)

    def good(self, name, det):
        """A call the context accepts, whatever was refused before it."""
        if name in ("five", "multi"):
            det.run(self.f32[:, :det.d_in].contiguous(), 2)
        elif name == "one":
            det.run_u8(self.x, capi.PIX_GRAY, 0, n=2)
        else:
            det.run_u8(self.x, capi.PIX_RGB, 0, n=2)
        det.synchronize()

    def close(self):
        for d in (self.three, self.one, self.five, self.odd, self.multi, self.turn):
            d.close()


def yuv(base, **kw):
    d = capi.YuvDesc.from_buffer_copy(base)
    for k, v in kw.items():
        plane, _, field = k.partition("_")
        if plane in ("y", "u", "v"):
            setattr(getattr(d, plane), field, v)
        else:
            setattr(d, k, v)
    return d


def image(base, **kw):
    d = capi.ImageDesc.from_buffer_copy(base)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def raw(det, fn, *args):
    """An entry by its C name (null pointers, counts the Python methods would not pass on)."""
    det._chk(getattr(det.lib, fn)(det.ctx, *args))


def rz_on(k, d):
    d.set_input_resize(SH, SW, SCALE)


def rz_off(k, d):
    d.set_input_resize(0, 0, 1.0)


def layout(chroma, stride):
    return lambda k, d: d.set_yuv_layout(chroma, stride)


INV, UNS, NOPLAN = capi.E_INVALID, capi.E_UNSUPPORTED, capi.E_NOPLAN
P = C.c_void_p
DBL = C.c_double

# id, context, call(k, det), code, piece of the message, (before, after) or None
ROWS = [
    # ---- what every pyramid entry checks first
    ("u8_no_plan", "bare", lambda k, d: d.run_u8(k.x, capi.PIX_RGB, 0, n=1), NOPLAN, "pyramid: plan first", None),
    ("image_no_plan", "bare", lambda k, d: d.run_image(k.ptr, 1, k.img), NOPLAN, "pyramid: plan first", None),
    ("yuv_no_plan", "bare", lambda k, d: d.run_yuv(k.x, 1, k.yuv), NOPLAN, "pyramid: plan first", None),
    ("yuv_resized_no_plan", "bare", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, SH, SW, SCALE), NOPLAN, "pyramid: plan first", None),
    ("image_resized_no_plan", "bare", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, SH, SW, SCALE), NOPLAN, "pyramid: plan first", None),
    ("u8_streams", "multi", lambda k, d: d.run_u8(k.x, capi.PIX_RGB, 0, n=2), UNS, "pyramid_u8: not available with option \"streams\" > 1", None),
    ("image_streams", "multi", lambda k, d: d.run_image(k.ptr, 2, k.img), UNS, "pyramid_image: not available with option \"streams\" > 1", None),
    ("image_resized_streams", "multi", lambda k, d: d.run_image_resized(k.ptr, 2, k.imgS, SH, SW, SCALE), UNS,
     "pyramid_image_resized: not available with option \"streams\" > 1", None),
    ("yuv_streams", "multi", lambda k, d: d.pyramid_yuv(k.x, 2, k.yuv), UNS, "pyramid_yuv: not available with option \"streams\" > 1", None),
    ("yuv_resized_streams", "multi", lambda k, d: d.run_yuv_resized(k.x, 2, k.yuvS, SH, SW, SCALE), UNS,
     "pyramid_yuv_resized: not available with option \"streams\" > 1", None),
    ("streams_before_the_description", "multi", lambda k, d: d.run_yuv(k.x, 2, yuv(k.yuv, sub_x=2)), UNS, "pyramid_yuv: not available", None),
    ("u8_no_frames", "three", lambda k, d: d.run_u8(k.x, capi.PIX_RGB, 0, n=0), INV, "pyramid: n_frames out of range", None),
    ("u8_too_many_frames", "three", lambda k, d: d.pyramid_u8(k.x, capi.PIX_RGB, 0, n=3), INV, "pyramid: n_frames out of range", None),
    ("u8_null_frames", "three", lambda k, d: raw(d, "acf_hip_run_u8", None, 1, capi.PIX_RGB, 0), INV, "pyramid: n_frames out of range", None),
    ("f32_null_frames", "three", lambda k, d: raw(d, "acf_hip_pyramid", None, 1), INV, "pyramid: n_frames out of range", None),
    ("image_too_many_frames", "three", lambda k, d: d.run_image(k.ptr, 3, k.img), INV, "pyramid: n_frames out of range", None),
    ("yuv_no_frames", "three", lambda k, d: d.run_yuv(k.x, 0, k.yuv), INV, "pyramid: n_frames out of range", None),
    ("yuv_resized_too_many_frames", "three", lambda k, d: d.run_yuv_resized(k.x, 3, k.yuvS, SH, SW, SCALE), INV, "pyramid: n_frames out of range", None),
    ("frames_before_the_description", "three", lambda k, d: d.run_image(k.ptr, 3, image(k.img, dtype=7)), INV, "pyramid: n_frames out of range", None),
    # ---- the 8-bit entry
    ("u8_five_planes", "five", lambda k, d: d.run_u8(k.x, capi.PIX_RGB, 0, n=1), INV, "pyramid_u8: a plan for five input planes (image + M, O) takes float frames", None),
    ("u8_five_planes_before_the_layout", "five", lambda k, d: d.run_u8(k.x, 99, 0, n=1), INV, "pyramid_u8: a plan for five input planes", None),
    ("u8_pixel_layout", "three", lambda k, d: d.run_u8(k.x, 99, 0, n=1), INV, "pyramid_u8: pixel layout", None),
    ("u8_negative_stride", "three", lambda k, d: d.run_u8(k.x, capi.PIX_RGB, -1, n=1), INV, "pyramid_u8: frame size", None),
    ("u8_short_stride", "three", lambda k, d: d.pyramid_u8(k.x, capi.PIX_RGBA, 4 * PW - 1, n=1), INV, "pyramid_u8: row stride smaller than a row", None),
    ("u8_stride_before_planes", "one", lambda k, d: d.run_u8(k.x, capi.PIX_RGB, 5, n=1), INV, "pyramid_u8: row stride smaller than a row", None),
    ("u8_nv12_odd_rows", "odd", lambda k, d: d.run_u8(k.x, capi.PIX_NV12, 0, n=1), INV, "pyramid_u8: NV12 / NV21 frames have even rows and columns", None),
    ("u8_chroma_inside_luma", "three", lambda k, d: d.run_u8(k.x, capi.PIX_NV12, 0, n=1), INV, "pyramid_u8: chroma offset inside the luma plane",
     (layout(PW, 0), layout(0, 0))),
    ("u8_frames_overlap", "three", lambda k, d: d.run_u8(k.x, capi.PIX_NV21, 0, n=2), INV, "pyramid_u8: frame stride smaller than a frame (frames would overlap)",
     (layout(0, PH * PW), layout(0, 0))),
    ("u8_colour_into_one_plane", "one", lambda k, d: d.run_u8(k.x, capi.PIX_BGR, 0, n=1), INV,
     "pyramid_u8: the plan's input planes (d) must be 3 for colour layouts (NV12 / NV21 included) and 1 for GRAY", None),
    ("u8_nv12_into_one_plane", "one", lambda k, d: d.run_u8(k.x, capi.PIX_NV12, 0, n=1), INV,
     "pyramid_u8: the plan's input planes (d) must be 3 for colour layouts (NV12 / NV21 included) and 1 for GRAY", None),
    ("u8_gray_into_three_planes", "three", lambda k, d: d.run_u8(k.x, capi.PIX_GRAY, 0, n=1), INV,
     "pyramid_u8: the plan's input planes (d) must be 3 for colour layouts (NV12 / NV21 included) and 1 for GRAY", None),
    ("u8_nv12_resize_into_one_plane", "one", lambda k, d: d.run_u8(k.x, capi.PIX_NV12, 0, n=1), INV,
     "pyramid_u8: the plan's input planes (d) must be 3 for NV12 / NV21", (rz_on, rz_off)),
    ("u8_nv12_resize_short_stride", "three", lambda k, d: d.run_u8(k.x, capi.PIX_NV12, SW - 2, n=1), INV, "pyramid_u8: row stride smaller than a row", (rz_on, rz_off)),
    ("u8_resize_short_stride", "three", lambda k, d: d.run_u8(k.x, capi.PIX_RGB, 3 * PW, n=1), INV,
     "pyramid_u8 (the unreduced frame): row stride smaller than a row", (rz_on, rz_off)),
    ("u8_resize_pixel_layout", "three", lambda k, d: d.run_u8(k.x, -1, 0, n=1), INV, "pyramid_u8 (the unreduced frame): pixel layout", (rz_on, rz_off)),
    ("u8_resize_gray_into_three_planes", "three", lambda k, d: d.run_u8(k.x, capi.PIX_GRAY, 0, n=1), INV,
     "pyramid_u8: the plan's input planes (d) must be 3 for colour layouts", (rz_on, rz_off)),
    # ---- the tensor entry
    ("image_null_frames", "three", lambda k, d: raw(d, "acf_hip_run_image", None, 1, C.byref(k.img)), INV, "pyramid_image: null frames or description", None),
    ("image_null_description", "three", lambda k, d: raw(d, "acf_hip_pyramid_image", P(k.ptr), 1, None), INV, "pyramid_image: null frames or description", None),
    ("image_null_before_streams", "multi", lambda k, d: raw(d, "acf_hip_run_image", None, 1, C.byref(k.img)), INV, "pyramid_image: null frames or description", None),
    ("image_dtype", "three", lambda k, d: d.run_image(k.ptr, 1, image(k.img, dtype=7)), INV, "pyramid_image: unknown dtype", None),
    ("image_two_channels", "three", lambda k, d: d.run_image(k.ptr, 1, image(k.img, channels=2)), INV, "pyramid_image: channels must be 1 or 3", None),
    ("image_stride_x", "three", lambda k, d: d.pyramid_image(k.ptr, 1, image(k.img, stride_x=0)), INV, "pyramid_image: stride_x and stride_y must be positive", None),
    ("image_stride_n", "three", lambda k, d: d.run_image(k.ptr, 1, image(k.img, stride_n=-1)), INV, "pyramid_image: negative stride_n", None),
    ("image_description_before_five_planes", "five", lambda k, d: d.run_image(k.ptr, 1, image(k.img, stride_y=-3)), INV,
     "pyramid_image: stride_x and stride_y must be positive", None),
    ("image_five_planes", "five", lambda k, d: d.run_image(k.ptr, 1, k.img), INV,
     "pyramid_image: a plan for five input planes (image + M, O) takes planar float frames", None),
    ("image_channels", "three", lambda k, d: d.run_image(k.ptr, 1, image(k.img, channels=1)), INV, "pyramid_image: channels must be the plan's input planes (d)", None),
    ("image_channels_into_one_plane", "one", lambda k, d: d.run_image(k.ptr, 1, k.img), INV, "pyramid_image: channels must be the plan's input planes (d)", None),
    ("image_with_input_resize", "three", lambda k, d: d.run_image(k.ptr, 1, k.img), INV,
     "pyramid_image: not with acf_hip_set_input_resize (the resize takes packed 8-bit frames)", (rz_on, rz_off)),
    ("image_channels_before_input_resize", "three", lambda k, d: d.run_image(k.ptr, 1, image(k.img, channels=1)), INV,
     "pyramid_image: channels must be the plan's input planes (d)", (rz_on, rz_off)),
    # ---- the resized tensor entry
    ("image_resized_null_frames", "three", lambda k, d: raw(d, "acf_hip_run_image_resized", None, 1, C.byref(k.imgS), SH, SW, DBL(SCALE)), INV,
     "pyramid_image_resized: null frames or description", None),
    ("image_resized_null_description", "three", lambda k, d: raw(d, "acf_hip_pyramid_image_resized", P(k.ptr), 1, None, SH, SW, DBL(SCALE)), INV,
     "pyramid_image_resized: null frames or description", None),
    ("image_resized_dtype_code", "three", lambda k, d: d.run_image_resized(k.ptr, 1, image(k.imgS, dtype=-1), SH, SW, SCALE), INV, "pyramid_image_resized: unknown dtype", None),
    ("image_resized_two_channels", "three", lambda k, d: d.run_image_resized(k.ptr, 1, image(k.imgS, channels=2), SH, SW, SCALE), INV,
     "pyramid_image_resized: channels must be 1 or 3", None),
    ("image_resized_stride_y", "three", lambda k, d: d.pyramid_image_resized(k.ptr, 1, image(k.imgS, stride_y=0), SH, SW, SCALE), INV,
     "pyramid_image_resized: stride_x and stride_y must be positive", None),
    ("image_resized_stride_n", "three", lambda k, d: d.run_image_resized(k.ptr, 1, image(k.imgS, stride_n=-1), SH, SW, SCALE), INV,
     "pyramid_image_resized: negative stride_n", None),
    ("image_resized_five_planes", "five", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, SH, SW, SCALE), INV,
     "pyramid_image_resized: a plan for five input planes (image + M, O) takes planar float frames", None),
    ("image_resized_channels", "one", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, SH, SW, SCALE), INV,
     "pyramid_image_resized: channels must be the plan's input planes (d)", None),
    ("image_resized_channels_before_dtype", "one", lambda k, d: d.run_image_resized(k.ptr, 1, image(k.imgS, dtype=capi.T_F16), SH, SW, SCALE), INV,
     "pyramid_image_resized: channels must be the plan's input planes (d)", None),
    ("image_resized_f16", "three", lambda k, d: d.run_image_resized(k.ptr, 1, image(k.imgS, dtype=capi.T_F16), SH, SW, SCALE), UNS,
     "pyramid_image_resized: dtype must be ACF_HIP_T_U8 (cv::resize's CV_32F arithmetic is not restated)", None),
    ("image_resized_dtype_before_the_size", "three", lambda k, d: d.pyramid_image_resized(k.ptr, 1, image(k.imgS, dtype=capi.T_F32), 0, SW, SCALE), UNS,
     "pyramid_image_resized: dtype must be ACF_HIP_T_U8", None),
    ("image_resized_no_rows", "three", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, 0, SW, SCALE), INV,
     "pyramid_image_resized: src_rows and src_cols >= 1, scale a positive finite number", None),
    ("image_resized_nan_scale", "three", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, SH, SW, NAN), INV,
     "pyramid_image_resized: src_rows and src_cols >= 1, scale a positive finite number", None),
    ("image_resized_with_input_resize", "three", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, SH, SW, SCALE), INV,
     "pyramid_image_resized: not with acf_hip_set_input_resize (the entry resizes by itself)", (rz_on, rz_off)),
    ("image_resized_size_before_input_resize", "three", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, SH, -SW, SCALE), INV,
     "pyramid_image_resized: src_rows and src_cols >= 1", (rz_on, rz_off)),
    ("image_resized_other_plan", "three", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, SH, SW, 0.75), INV,
     "pyramid_image_resized: the plan must be for the reduced size (acf_hip_resize_dims of the frame size and scale)", None),
    ("image_resized_input_resize_before_the_plan", "three", lambda k, d: d.run_image_resized(k.ptr, 1, k.imgS, SH + 2, SW, SCALE), INV,
     "pyramid_image_resized: not with acf_hip_set_input_resize", (rz_on, rz_off)),
    # ---- the YUV entry
    ("yuv_null_base", "three", lambda k, d: raw(d, "acf_hip_run_yuv", None, 1, C.byref(k.yuv)), INV, "pyramid_yuv: null base or description", None),
    ("yuv_null_description", "three", lambda k, d: raw(d, "acf_hip_pyramid_yuv", P(k.ptr), 1, None), INV, "pyramid_yuv: null base or description", None),
    ("yuv_sub_x", "three", lambda k, d: d.run_yuv(k.x, 1, yuv(k.yuv, sub_x=2)), INV, "pyramid_yuv: sub_x and sub_y must be 0 or 1", None),
    ("yuv_stride_px", "three", lambda k, d: d.pyramid_yuv(k.x, 1, yuv(k.yuv, u_stride_px=0)), INV, "pyramid_yuv: stride_px and stride_row must be positive", None),
    ("yuv_stride_n", "three", lambda k, d: d.run_yuv(k.x, 1, yuv(k.yuv, v_stride_n=-4)), INV, "pyramid_yuv: negative stride_n", None),
    ("yuv_one_plane", "one", lambda k, d: d.run_yuv(k.x, 1, k.yuv), INV, "pyramid_yuv: the plan's input planes (d) must be 3", None),
    ("yuv_five_planes", "five", lambda k, d: d.run_yuv(k.x, 1, k.yuv), INV, "pyramid_yuv: the plan's input planes (d) must be 3", None),
    ("yuv_description_before_planes", "five", lambda k, d: d.run_yuv(k.x, 1, yuv(k.yuv, sub_y=-1)), INV, "pyramid_yuv: sub_x and sub_y must be 0 or 1", None),
    ("yuv_with_input_resize", "three", lambda k, d: d.run_yuv(k.x, 1, k.yuv), INV,
     "pyramid_yuv: not with acf_hip_set_input_resize (the resize takes the 8-bit entries' frames)", (rz_on, rz_off)),
    # ---- the resized YUV entry
    ("yuv_resized_null_base", "three", lambda k, d: raw(d, "acf_hip_run_yuv_resized", None, 1, C.byref(k.yuvS), SH, SW, DBL(SCALE)), INV,
     "pyramid_yuv_resized: null base or description", None),
    ("yuv_resized_null_description", "three", lambda k, d: raw(d, "acf_hip_pyramid_yuv_resized", P(k.ptr), 1, None, SH, SW, DBL(SCALE)), INV,
     "pyramid_yuv_resized: null base or description", None),
    ("yuv_resized_sub_y", "three", lambda k, d: d.run_yuv_resized(k.x, 1, yuv(k.yuvS, sub_y=2), SH, SW, SCALE), INV, "pyramid_yuv_resized: sub_x and sub_y must be 0 or 1", None),
    ("yuv_resized_stride_row", "three", lambda k, d: d.pyramid_yuv_resized(k.x, 1, yuv(k.yuvS, u_stride_row=0), SH, SW, SCALE), INV,
     "pyramid_yuv_resized: stride_px and stride_row must be positive", None),
    ("yuv_resized_stride_n", "three", lambda k, d: d.run_yuv_resized(k.x, 1, yuv(k.yuvS, y_stride_n=-1), SH, SW, SCALE), INV, "pyramid_yuv_resized: negative stride_n", None),
    ("yuv_resized_one_plane", "one", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, SH, SW, SCALE), INV, "pyramid_yuv_resized: the plan's input planes (d) must be 3", None),
    ("yuv_resized_five_planes", "five", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, SH, SW, SCALE), INV, "pyramid_yuv_resized: the plan's input planes (d) must be 3", None),
    ("yuv_resized_planes_before_the_size", "one", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, 0, 0, SCALE), INV, "pyramid_yuv_resized: the plan's input planes (d) must be 3", None),
    ("yuv_resized_no_cols", "three", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, SH, 0, SCALE), INV,
     "pyramid_yuv_resized: src_rows and src_cols >= 1, scale a positive finite number", None),
    ("yuv_resized_inf_scale", "three", lambda k, d: d.pyramid_yuv_resized(k.x, 1, k.yuvS, SH, SW, INF), INV,
     "pyramid_yuv_resized: src_rows and src_cols >= 1, scale a positive finite number", None),
    ("yuv_resized_negative_scale", "three", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, SH, SW, -0.5), INV, "pyramid_yuv_resized: src_rows and src_cols >= 1", None),
    ("yuv_resized_with_input_resize", "three", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, SH, SW, SCALE), INV,
     "pyramid_yuv_resized: not with acf_hip_set_input_resize (the entry resizes by itself)", (rz_on, rz_off)),
    ("yuv_resized_other_plan", "three", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, SH + 2, SW, SCALE), INV,
     "pyramid_yuv_resized: the plan must be for the reduced size (acf_hip_resize_dims of the frame size and scale)", None),
    ("yuv_resized_scale_one", "three", lambda k, d: d.run_yuv_resized(k.x, 1, k.yuvS, SH, SW, 1.0), INV, "pyramid_yuv_resized: the plan must be for the reduced size", None),
    # ---- the settings in front of the entries, the conversion alone
    ("input_resize_no_plan", "bare", lambda k, d: d.set_input_resize(SH, SW, SCALE), NOPLAN, "set_input_resize: plan first (for the reduced size, acf_hip_resize_dims)", None),
    ("input_resize_streams", "multi", lambda k, d: d.set_input_resize(SH, SW, SCALE), UNS,
     "set_input_resize: not with option \"streams\" > 1; before acf_hip_stream_open", None),
    ("input_resize_other_plan", "three", lambda k, d: d.set_input_resize(SH, SW, 0.75), INV,
     "set_input_resize: the plan must be for the reduced size (acf_hip_resize_dims of the frame size and scale)", None),
    ("input_resize_nan_scale", "three", lambda k, d: d.set_input_resize(SH, SW, NAN), INV, "set_input_resize: the plan must be for the reduced size", None),
    ("yuv_layout_no_plan", "bare", lambda k, d: d.set_yuv_layout(0, 0), NOPLAN, "set_yuv_layout: plan first", None),
    ("yuv_layout_streams", "multi", lambda k, d: d.set_yuv_layout(0, 0), UNS, "set_yuv_layout: not with option \"streams\" > 1; before acf_hip_stream_open", None),
    ("yuv_layout_negative", "three", lambda k, d: d.set_yuv_layout(-1, 0), INV, "set_yuv_layout: negative offset or stride", None),
    ("yuv_to_rgb8_null", "three", lambda k, d: raw(d, "acf_hip_yuv_to_rgb8", P(k.ptr), 1, PH, PW, C.byref(k.yuv), None), INV,
     "yuv_to_rgb8: null base, description or destination", None),
    ("yuv_to_rgb8_description", "three", lambda k, d: raw(d, "acf_hip_yuv_to_rgb8", P(k.ptr), 1, PH, PW, C.byref(yuv(k.yuv, sub_x=-1)), P(k.buf.data_ptr())), INV,
     "yuv_to_rgb8: sub_x and sub_y must be 0 or 1", None),
    ("yuv_to_rgb8_frames", "three", lambda k, d: raw(d, "acf_hip_yuv_to_rgb8", P(k.ptr), 65536, 2, 2, C.byref(k.yuv), P(k.buf.data_ptr())), INV,
     "yuv_to_rgb8: n_frames 1 .. 65535, rows and cols >= 1", None),
    ("yuv_to_rgb8_rows", "three", lambda k, d: raw(d, "acf_hip_yuv_to_rgb8", P(k.ptr), 1, 0, PW, C.byref(k.yuv), P(k.buf.data_ptr())), INV,
     "yuv_to_rgb8: n_frames 1 .. 65535, rows and cols >= 1", None),
    # ---- stream_open
    ("stream_no_plan", "bare", lambda k, d: d.stream_open(capi.PIX_RGB, 0, 64, 2), NOPLAN, "stream_open: plan first", None),
    ("stream_streams", "multi", lambda k, d: d.stream_open(capi.PIX_RGB, 0, 64, 2), UNS, "stream_open: not available with option \"streams\" > 1", None),
    ("stream_depth", "three", lambda k, d: d.stream_open(capi.PIX_RGB, 0, 64, 1), INV, "stream_open: depth must be 2..8, cap > 0", None),
    ("stream_cap", "three", lambda k, d: d.stream_open(capi.PIX_RGB, 0, 0, 2), INV, "stream_open: depth must be 2..8, cap > 0", None),
    ("stream_depth_before_the_layout", "three", lambda k, d: d.stream_open(99, 0, 64, 9), INV, "stream_open: depth must be 2..8, cap > 0", None),
    ("stream_pixel_layout", "three", lambda k, d: d.stream_open(99, 0, 64, 2), INV, "stream_open: pixel layout", None),
    ("stream_short_stride", "three", lambda k, d: d.stream_open(capi.PIX_RGB, PW, 64, 2), INV, "stream_open: row stride smaller than a row", None),
    ("stream_resize_short_stride", "three", lambda k, d: d.stream_open(capi.PIX_RGB, 3 * PW, 64, 2), INV, "stream_open: row stride smaller than a row", (rz_on, rz_off)),
    ("stream_nv12_odd_rows", "odd", lambda k, d: d.stream_open(capi.PIX_NV21, 0, 64, 2), INV, "stream_open: NV12 / NV21 frames have even rows and columns", None),
    ("stream_chroma_inside_luma", "three", lambda k, d: d.stream_open(capi.PIX_NV12, 0, 64, 2), INV, "stream_open: chroma offset inside the luma plane",
     (layout(8, 0), layout(0, 0))),
    ("stream_gray_into_three_planes", "three", lambda k, d: d.stream_open(capi.PIX_GRAY, 0, 64, 2), INV,
     "stream_open: the plan's input planes (d) must be 3 for colour layouts (NV12 / NV21 included) and 1 for GRAY", None),
    ("stream_nv12_into_one_plane", "one", lambda k, d: d.stream_open(capi.PIX_NV12, 0, 64, 2), INV,
     "stream_open: the plan's input planes (d) must be 3 for colour layouts (NV12 / NV21 included) and 1 for GRAY", None),
    # ---- stream_open_yuv
    ("stream_yuv_no_plan", "bare", lambda k, d: d.stream_open_yuv(k.yuv, k.fb, 64, 2), NOPLAN, "stream_open_yuv: plan first", None),
    ("stream_yuv_streams", "multi", lambda k, d: d.stream_open_yuv(k.yuv, k.fb, 64, 2), UNS, "stream_open_yuv: not available with option \"streams\" > 1", None),
    ("stream_yuv_depth", "three", lambda k, d: d.stream_open_yuv(k.yuv, k.fb, 64, 9), INV, "stream_open_yuv: depth must be 2..8, cap > 0", None),
    ("stream_yuv_null_description", "three", lambda k, d: raw(d, "acf_hip_stream_open_yuv", None, C.c_int64(k.fb), 64, 2), INV, "stream_open_yuv: null description", None),
    ("stream_yuv_depth_before_the_description", "three", lambda k, d: d.stream_open_yuv(yuv(k.yuv, sub_x=2), k.fb, 0, 2), INV, "stream_open_yuv: depth must be 2..8, cap > 0", None),
    ("stream_yuv_sub_x", "three", lambda k, d: d.stream_open_yuv(yuv(k.yuv, sub_x=2), k.fb, 64, 2), INV, "stream_open_yuv: sub_x and sub_y must be 0 or 1", None),
    ("stream_yuv_stride_px", "three", lambda k, d: d.stream_open_yuv(yuv(k.yuv, y_stride_px=0), k.fb, 64, 2), INV, "stream_open_yuv: stride_px and stride_row must be positive", None),
    ("stream_yuv_negative_stride_n", "three", lambda k, d: d.stream_open_yuv(yuv(k.yuv, u_stride_n=-1), k.fb, 64, 2), INV, "stream_open_yuv: negative stride_n", None),
    ("stream_yuv_one_plane", "one", lambda k, d: d.stream_open_yuv(k.yuv, k.fb, 64, 2), INV,
     "stream_open_yuv: the plan's input planes (d) must be 3, and not with acf_hip_set_input_resize", None),
    ("stream_yuv_with_input_resize", "three", lambda k, d: d.stream_open_yuv(k.yuv, k.fb, 64, 2), INV,
     "stream_open_yuv: the plan's input planes (d) must be 3, and not with acf_hip_set_input_resize", (rz_on, rz_off)),
    ("stream_yuv_plane_outside", "three", lambda k, d: d.stream_open_yuv(k.yuv, k.fb - 1, 64, 2), INV, "stream_open_yuv: every plane of a frame must lie in [0, frame_bytes)", None),
    ("stream_yuv_plane_below", "three", lambda k, d: d.stream_open_yuv(yuv(k.yuv, v_offset=-8), k.fb, 64, 2), INV,
     "stream_open_yuv: every plane of a frame must lie in [0, frame_bytes)", None),
    ("stream_yuv_stride_n", "three", lambda k, d: d.stream_open_yuv(yuv(k.yuv, y_stride_n=k.fb + 4), k.fb, 64, 2), INV,
     "stream_open_yuv: stride_n of every plane must be frame_bytes", None),
    ("stream_yuv_extent_before_stride_n", "three", lambda k, d: d.stream_open_yuv(yuv(k.yuv, u_stride_n=k.fb + 4, v_offset=k.fb), k.fb, 64, 2), INV,
     "stream_open_yuv: every plane of a frame must lie in", None),
    # ---- stream_open_yuv_resized
    ("stream_yuv_resized_no_plan", "bare", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS, SH, SW, SCALE, 64, 2), NOPLAN, "stream_open_yuv_resized: plan first", None),
    ("stream_yuv_resized_streams", "multi", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS, SH, SW, SCALE, 64, 2), UNS,
     "stream_open_yuv_resized: not available with option \"streams\" > 1", None),
    ("stream_yuv_resized_cap", "three", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS, SH, SW, SCALE, 0, 2), INV, "stream_open_yuv_resized: depth must be 2..8, cap > 0", None),
    ("stream_yuv_resized_null_description", "three", lambda k, d: raw(d, "acf_hip_stream_open_yuv_resized", None, C.c_int64(k.fbS), SH, SW, DBL(SCALE), 64, 2), INV,
     "stream_open_yuv_resized: null description", None),
    ("stream_yuv_resized_sub_y", "three", lambda k, d: d.stream_open_yuv_resized(yuv(k.yuvS, sub_y=-1), k.fbS, SH, SW, SCALE, 64, 2), INV,
     "stream_open_yuv_resized: sub_x and sub_y must be 0 or 1", None),
    ("stream_yuv_resized_five_planes", "five", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS, SH, SW, SCALE, 64, 2), INV,
     "stream_open_yuv_resized: the plan's input planes (d) must be 3, and not with acf_hip_set_input_resize", None),
    ("stream_yuv_resized_with_input_resize", "three", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS, SH, SW, SCALE, 64, 2), INV,
     "stream_open_yuv_resized: the plan's input planes (d) must be 3, and not with acf_hip_set_input_resize", (rz_on, rz_off)),
    ("stream_yuv_resized_no_rows", "three", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS, 0, SW, SCALE, 64, 2), INV,
     "stream_open_yuv_resized: src_rows and src_cols >= 1, scale a positive finite number", None),
    ("stream_yuv_resized_zero_scale", "three", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS, SH, SW, 0.0, 64, 2), INV,
     "stream_open_yuv_resized: src_rows and src_cols >= 1, scale a positive finite number", None),
    ("stream_yuv_resized_other_plan", "three", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS, SH, SW, 0.75, 64, 2), INV,
     "stream_open_yuv_resized: the plan must be for the reduced size (acf_hip_resize_dims of the frame size and scale)", None),
    ("stream_yuv_resized_plan_before_the_extent", "three", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS - 1, SH + 2, SW, SCALE, 64, 2), INV,
     "stream_open_yuv_resized: the plan must be for the reduced size", None),
    ("stream_yuv_resized_plane_outside", "three", lambda k, d: d.stream_open_yuv_resized(k.yuvS, k.fbS - 1, SH, SW, SCALE, 64, 2), INV,
     "stream_open_yuv_resized: every plane of a frame must lie in [0, frame_bytes)", None),
    ("stream_yuv_resized_room_for_the_plan_size_only", "three", lambda k, d: d.stream_open_yuv_resized(yuv(k.yuvS, y_stride_n=k.fb, u_stride_n=k.fb, v_stride_n=k.fb), k.fb, SH, SW, SCALE, 64, 2),
     INV, "stream_open_yuv_resized: every plane of a frame must lie in [0, frame_bytes)", None),
    ("stream_yuv_resized_stride_n", "three", lambda k, d: d.stream_open_yuv_resized(yuv(k.yuvS, v_stride_n=k.fbS + 4), k.fbS, SH, SW, SCALE, 64, 2), INV,
     "stream_open_yuv_resized: stride_n of every plane must be frame_bytes", None),
]


# ---- the oriented, the oriented resized and the video families, by their C names.  An argument is a value or a function of the contexts.
def ent(fn, *args):
    return lambda k, d: raw(d, "acf_hip_" + fn, *[a(k) if callable(a) else a for a in args])


PTR = lambda k: P(k.ptr)
ODD = lambda k: P(k.ptr + 1)
I, IS = (lambda k: C.byref(k.img)), (lambda k: C.byref(k.imgS))
Y, YS, Y10 = (lambda k: C.byref(k.yuv)), (lambda k: C.byref(k.yuvS)), (lambda k: C.byref(k.yuv10))
FB, FBS, FB10 = (lambda k: k.fb), (lambda k: k.fbS), (lambda k: k.fb10)
F709, F10 = (lambda k: C.byref(k.f709)), (lambda k: C.byref(k.f10))


def ydesc(which, **kw):
    return lambda k: C.byref(yuv(getattr(k, which), **{f: (v(k) if callable(v) else v) for f, v in kw.items()}))


def idesc(which, **kw):
    return lambda k: C.byref(image(getattr(k, which), **kw))


def fmt(*v):
    return lambda k: C.byref(capi.YuvFormat(*(list(v) + [0, 0, 0])[:4]))


ORIENT = "orient must be 0 .. 7 (ACF_HIP_ORIENT_*), src_rows and src_cols >= 1"
UPRIGHT = "the plan must be for the upright size (acf_hip_oriented_dims of the frame size and orientation)"
REDUCED = "the plan must be for the reduced size (acf_hip_resize_dims of the frame size and scale)"
SIZE_SCALE = "src_rows and src_cols >= 1, scale a positive finite number"
VSCALE = "scale must be 0 (no resize) or a positive finite number"
WIDE = "more than 8 bits a sample: upright and unreduced frames only (orient 0, scale 0)"
STREAMS = "not available with option \"streams\" > 1"
FRAMES = "pyramid: n_frames out of range"
RZ_YUV = "not with acf_hip_set_input_resize (the resize takes the 8-bit entries' frames)"
RZ_IMAGE = "not with acf_hip_set_input_resize (the resize takes packed 8-bit frames)"
RZ_SELF = "not with acf_hip_set_input_resize (the entry resizes by itself)"
YUV_PLANES = "the plan's input planes (d) must be 3"
OPEN_PLANES = "the plan's input planes (d) must be 3, and not with acf_hip_set_input_resize"
IMAGE_FIVE = "a plan for five input planes (image + M, O) takes planar float frames"
CHANNELS = "channels must be the plan's input planes (d)"
DEPTH = "depth must be 2..8, cap > 0"
INSIDE = "every plane of a frame must lie in [0, frame_bytes)"
STRIDE_N = "stride_n of every plane must be frame_bytes"
EVEN = "16-bit samples need even offsets and strides"
BAD_FORMATS = [((7,), "bits must be 8 .. 16"), ((17,), "bits must be 8 .. 16"), ((8, 1), "shift must be 0 for 8 bits, and shift + bits <= 16"),
               ((10, 7), "shift must be 0 for 8 bits, and shift + bits <= 16"), ((16, 1), "shift must be 0 for 8 bits, and shift + bits <= 16"),
               ((8, 0, 3), "unknown matrix (ACF_HIP_YUV_MATRIX_*)"), ((8, 0, 0, 2), "full_range must be 0 or 1")]
RZ = (rz_on, rz_off)
FAMILY_ROWS = []


def fam(prefix, who, rows):
    """rows of (id, context, call, code, reason, around): the piece is `who: reason`, or the reason alone where who is None or the reason
    names its entry itself (a forwarded call; "pyramid: ...")."""
    for rid, ctx, call, code, reason, around in rows:
        own = who is not None and not reason.startswith("pyramid: ")
        FAMILY_ROWS.append((prefix + "_" + rid, ctx, call, code, (who + ": " + reason) if own else reason, around))


def oriented(kind, fn, FR, D, dvar, null, planes_one, planes_five, rz_text, bad_desc, bad_text):
    """acf_hip_run_<kind>_oriented(ctx, frames, n, desc, src_rows, src_cols, orient); FR: the frames, D: the description of 96 x 128 frames"""
    e = lambda *a: ent(fn, *a)
    who = "pyramid_%s_oriented" % kind
    fam(kind + "_oriented", who, [
        ("null_frames", "three", e(None, 1, D, PH, PW, 2), INV, null, None),
        ("null_description", "three", ent(fn.replace("run_", "pyramid_"), FR, 1, None, PH, PW, 2), INV, null, None),
        ("orient_below", "three", e(FR, 1, D, PH, PW, -1), INV, ORIENT, None),
        ("orient_above", "three", e(FR, 1, D, PH, PW, 8), INV, ORIENT, None),
        ("no_rows", "three", e(FR, 1, D, 0, PW, 2), INV, ORIENT, None),
        ("negative_cols", "three", e(FR, 1, D, PH, -1, 2), INV, ORIENT, None),
        ("size_code_1", "three", e(FR, 1, D, PH, PW, 1), INV, UPRIGHT, None),
        ("size_code_2", "three", e(FR, 1, D, PH + 2, PW, 2), INV, UPRIGHT, None),
        ("size_code_5_quarter_turn", "turn", e(FR, 1, D, PH, PW + 2, 5), INV, UPRIGHT, None),
        ("one_plane", "one", e(FR, 1, D, PH, PW, 2), INV, planes_one, None),
        ("five_planes", "five", e(FR, 1, D, PH, PW, 2), INV, planes_five, None),
        ("with_input_resize", "three", e(FR, 1, D, PH, PW, 2), INV, rz_text, RZ),
        ("streams", "multi", e(FR, 2, D, PH, PW, 2), UNS, STREAMS, None),
        ("no_plan", "bare", e(FR, 1, D, PH, PW, 2), NOPLAN, "pyramid: plan first", None),
        ("no_frames", "three", e(FR, 0, D, PH, PW, 2), INV, FRAMES, None),
        ("too_many_frames", "turn", e(FR, 3, D, PH, PW, 1), INV, FRAMES, None),
        ("orient_before_plan_first", "bare", e(FR, 1, D, PH, PW, 8), INV, ORIENT, None),
        ("orient_before_null", "three", e(None, 1, D, PH, PW, -1), INV, ORIENT, None),
        ("null_before_streams", "multi", e(None, 1, D, PH, PW, 2), INV, null, None),
        ("streams_before_frames", "multi", e(FR, 0, D, PH, PW, 2), UNS, STREAMS, None),
        ("frames_before_description", "three", e(FR, 3, bad_desc, PH, PW, 2), INV, FRAMES, None),
        ("description_before_planes", "five", e(FR, 1, bad_desc, PH, PW, 2), INV, bad_text, None),
        ("planes_before_input_resize", "one", e(FR, 1, D, PH, PW, 2), INV, planes_one, RZ),
        ("input_resize_before_size", "three", e(FR, 1, D, PH + 2, PW, 2), INV, rz_text, RZ),
    ])
    fam(kind + "_oriented_code_0", None, [   # (code 0 is the un-oriented entry, whichever name the message carries)
        ("size", "three", e(FR, 1, D, PH + 2, PW, 0), INV, UPRIGHT, None),
        ("one_plane", "one", e(FR, 1, D, PH, PW, 0), INV, planes_one, None),
        ("with_input_resize", "three", e(FR, 1, D, PH, PW, 0), INV, rz_text, RZ),
    ])


def oriented_resized(kind, fn, FR, D, dvar, null, planes_one, planes_five, bad_desc, bad_text):
    """acf_hip_run_<kind>_oriented_resized(ctx, frames, n, desc, src_rows, src_cols, orient, scale); D: the description of 192 x 256 frames"""
    e = lambda *a: ent(fn, *a)
    who = "pyramid_%s_oriented_resized" % kind
    fam(kind + "_oriented_resized", who, [
        ("null_frames", "three", e(None, 1, D, SH, SW, 2, SCALE), INV, null, None),
        ("null_description", "three", ent(fn.replace("run_", "pyramid_"), FR, 1, None, SH, SW, 2, SCALE), INV, null, None),
        ("orient_below", "three", e(FR, 1, D, SH, SW, -1, SCALE), INV, ORIENT, None),
        ("orient_above", "three", e(FR, 1, D, SH, SW, 8, SCALE), INV, ORIENT, None),
        ("no_rows", "three", e(FR, 1, D, 0, SW, 2, SCALE), INV, ORIENT, None),
        ("negative_cols", "three", e(FR, 1, D, SH, -1, 2, SCALE), INV, ORIENT, None),
        ("size_code_1", "three", e(FR, 1, D, SH, SW, 1, SCALE), INV, REDUCED, None),
        ("size_code_2", "three", e(FR, 1, D, SH + 2, SW, 2, SCALE), INV, REDUCED, None),
        ("size_code_7_quarter_turn", "turn", e(FR, 1, D, SH, SW + 2, 7, SCALE), INV, REDUCED, None),
        ("nan_scale", "three", e(FR, 1, D, SH, SW, 2, NAN), INV, SIZE_SCALE, None),
        ("negative_scale", "three", e(FR, 1, D, SH, SW, 2, -0.5), INV, SIZE_SCALE, None),
        ("zero_scale", "three", e(FR, 1, D, SH, SW, 2, 0.0), INV, SIZE_SCALE, None),
        ("other_plan", "three", e(FR, 1, D, SH, SW, 2, 0.75), INV, REDUCED, None),
        ("one_plane", "one", e(FR, 1, D, SH, SW, 2, SCALE), INV, planes_one, None),
        ("five_planes", "five", e(FR, 1, D, SH, SW, 2, SCALE), INV, planes_five, None),
        ("with_input_resize", "three", e(FR, 1, D, SH, SW, 2, SCALE), INV, RZ_SELF, RZ),
        ("streams", "multi", e(FR, 2, D, SH, SW, 2, SCALE), UNS, STREAMS, None),
        ("no_plan", "bare", e(FR, 1, D, SH, SW, 2, SCALE), NOPLAN, "pyramid: plan first", None),
        ("no_frames", "three", e(FR, 0, D, SH, SW, 2, SCALE), INV, FRAMES, None),
        ("too_many_frames", "turn", e(FR, 3, D, SH, SW, 1, SCALE), INV, FRAMES, None),
        ("orient_before_plan_first", "bare", e(FR, 1, D, SH, SW, 8, SCALE), INV, ORIENT, None),
        ("orient_before_null", "three", e(None, 1, D, SH, SW, -1, SCALE), INV, ORIENT, None),
        ("null_before_streams", "multi", e(None, 1, D, SH, SW, 2, SCALE), INV, null, None),
        ("frames_before_description", "three", e(FR, 3, bad_desc, SH, SW, 2, SCALE), INV, FRAMES, None),
        ("description_before_planes", "five", e(FR, 1, bad_desc, SH, SW, 2, SCALE), INV, bad_text, None),
        ("planes_before_scale", "one", e(FR, 1, D, SH, SW, 2, NAN), INV, planes_one, None),
        ("scale_before_input_resize", "three", e(FR, 1, D, SH, SW, 2, NAN), INV, SIZE_SCALE, RZ),
        ("input_resize_before_the_plan", "three", e(FR, 1, D, SH + 2, SW, 2, SCALE), INV, RZ_SELF, RZ),
    ])
    fam(kind + "_oriented_resized_code_0", None, [   # (code 0 is the resized entry)
        ("size", "three", e(FR, 1, D, SH + 2, SW, 0, SCALE), INV, REDUCED, None),
        ("nan_scale", "three", e(FR, 1, D, SH, SW, 0, NAN), INV, SIZE_SCALE, None),
        ("one_plane", "one", e(FR, 1, D, SH, SW, 0, SCALE), INV, planes_one, None),
        ("with_input_resize", "three", e(FR, 1, D, SH, SW, 0, SCALE), INV, RZ_SELF, RZ),
    ])


NULL_IMAGE, NULL_YUV = "null frames or description", "null base or description"
oriented("image", "run_image_oriented", PTR, I, "img", NULL_IMAGE, CHANNELS, IMAGE_FIVE, RZ_IMAGE, idesc("img", stride_y=-3), "stride_x and stride_y must be positive")
oriented("yuv", "run_yuv_oriented", PTR, Y, "yuv", NULL_YUV, YUV_PLANES, YUV_PLANES, RZ_YUV, ydesc("yuv", sub_y=-1), "sub_x and sub_y must be 0 or 1")
oriented_resized("image", "run_image_oriented_resized", PTR, IS, "imgS", NULL_IMAGE, CHANNELS, IMAGE_FIVE, idesc("imgS", stride_y=-3),
                 "stride_x and stride_y must be positive")
oriented_resized("yuv", "run_yuv_oriented_resized", PTR, YS, "yuvS", NULL_YUV, YUV_PLANES, YUV_PLANES, ydesc("yuvS", sub_y=-1), "sub_x and sub_y must be 0 or 1")
DTYPE = "dtype must be ACF_HIP_T_U8 (cv::resize's CV_32F arithmetic is not restated)"
fam("image_oriented_resized", "pyramid_image_oriented_resized", [
    ("f16", "three", ent("run_image_oriented_resized", PTR, 1, idesc("imgS", dtype=capi.T_F16), SH, SW, 2, SCALE), UNS, DTYPE, None),
    ("channels_before_dtype", "one", ent("run_image_oriented_resized", PTR, 1, idesc("imgS", dtype=capi.T_F16), SH, SW, 2, SCALE), INV, CHANNELS, None),
    ("dtype_before_scale", "three", ent("pyramid_image_oriented_resized", PTR, 1, idesc("imgS", dtype=capi.T_F32), SH, SW, 2, NAN), UNS, DTYPE, None),
    ("orient_before_dtype", "three", ent("run_image_oriented_resized", PTR, 1, idesc("imgS", dtype=capi.T_F32), SH, SW, 9, SCALE), INV, ORIENT, None),
])


def video(tag, FM, D, FR):
    """acf_hip_pyramid_video / run_video(ctx, base, n, desc, fmt, src_rows, src_cols, orient, scale) with a format other than the default:
    the rows the 8-bit and the 10-bit format share.  Plain: sizes 0, orient 0, scale 0."""
    e = lambda *a: ent("run_video", *a)
    p = lambda *a: ent("pyramid_video", *a)
    fam("video_" + tag, "pyramid_video", [
        ("null_base", "three", e(None, 1, D, FM, 0, 0, 0, 0.0), INV, NULL_YUV, None),
        ("null_description", "three", p(FR, 1, None, FM, 0, 0, 0, 0.0), INV, NULL_YUV, None),
        ("no_rows", "three", e(FR, 1, D, FM, 0, PW, 0, 0.0), INV, ORIENT, None),
        ("negative_cols", "three", e(FR, 1, D, FM, PH, -1, 0, 0.0), INV, ORIENT, None),
        ("size_code_0", "three", e(FR, 1, D, FM, PH + 2, PW, 0, 0.0), INV, UPRIGHT, None),
        ("nan_scale", "three", p(FR, 1, D, FM, SH, SW, 0, NAN), INV, VSCALE, None),
        ("negative_scale", "three", p(FR, 1, D, FM, SH, SW, 0, -0.5), INV, VSCALE, None),
        ("inf_scale", "three", p(FR, 1, D, FM, 0, 0, 0, INF), INV, VSCALE, None),
        ("one_plane", "one", e(FR, 1, D, FM, 0, 0, 0, 0.0), INV, YUV_PLANES, None),
        ("five_planes", "five", e(FR, 1, D, FM, 0, 0, 0, 0.0), INV, YUV_PLANES, None),
        ("with_input_resize", "three", e(FR, 1, D, FM, 0, 0, 0, 0.0), INV, RZ_YUV, RZ),
        ("streams", "multi", e(FR, 2, D, FM, 0, 0, 0, 0.0), UNS, STREAMS, None),
        ("no_plan", "bare", e(FR, 1, D, FM, 0, 0, 0, 0.0), NOPLAN, "pyramid: plan first", None),
        ("no_frames", "three", e(FR, 0, D, FM, 0, 0, 0, 0.0), INV, FRAMES, None),
        ("too_many_frames", "three", p(FR, 3, D, FM, PH, PW, 0, 0.0), INV, FRAMES, None),
        ("scale_before_orient", "three", p(FR, 1, D, FM, PH, PW, 8, NAN), INV, VSCALE, None),
        ("orient_before_null", "three", e(None, 1, D, FM, 0, PW, 0, 0.0), INV, ORIENT, None),
        ("scale_before_plan_first", "bare", p(FR, 1, D, FM, 0, 0, 0, -1.0), INV, VSCALE, None),
        ("null_before_streams", "multi", e(None, 1, D, FM, 0, 0, 0, 0.0), INV, NULL_YUV, None),
        ("frames_before_description", "three", e(FR, 3, ydesc("yuv", sub_x=2), FM, 0, 0, 0, 0.0), INV, FRAMES, None),
        ("description_before_planes", "five", e(FR, 1, ydesc("yuv", sub_x=2), FM, 0, 0, 0, 0.0), INV, "sub_x and sub_y must be 0 or 1", None),
        ("planes_before_input_resize", "one", e(FR, 1, D, FM, 0, 0, 0, 0.0), INV, YUV_PLANES, RZ),
    ])
    fam("video_" + tag, "run_video", [   # (what run_video checks before it goes the way of pyramid_video names itself)
        ("run_nan_scale", "three", e(FR, 1, D, FM, 0, 0, 0, NAN), INV, VSCALE, None),
    ])


video("bt709", F709, Y, PTR)
video("10_bits", F10, Y10, PTR)
fam("video_bt709", "pyramid_video", [
    ("orient_below", "three", ent("run_video", PTR, 1, Y, F709, PH, PW, -1, 0.0), INV, ORIENT, None),
    ("orient_above", "three", ent("run_video", PTR, 1, Y, F709, PH, PW, 8, 0.0), INV, ORIENT, None),
    ("orient_above_reduced", "three", ent("run_video", PTR, 1, YS, F709, SH, SW, 8, SCALE), INV, ORIENT, None),
    ("no_rows_reduced", "three", ent("run_video", PTR, 1, YS, F709, 0, SW, 0, SCALE), INV, ORIENT, None),
    ("size_code_1", "three", ent("run_video", PTR, 1, Y, F709, PH, PW, 1, 0.0), INV, UPRIGHT, None),
    ("size_code_2", "three", ent("run_video", PTR, 1, Y, F709, PH + 2, PW, 2, 0.0), INV, UPRIGHT, None),
    ("size_code_3_quarter_turn", "turn", ent("run_video", PTR, 1, Y, F709, PH, PW + 2, 3, 0.0), INV, UPRIGHT, None),
    ("other_plan", "three", ent("run_video", PTR, 1, YS, F709, SH, SW, 0, 0.75), INV, REDUCED, None),
    ("other_plan_code_1", "three", ent("run_video", PTR, 1, YS, F709, SH, SW, 1, SCALE), INV, REDUCED, None),
    ("reduced_with_input_resize", "three", ent("run_video", PTR, 1, YS, F709, SH, SW, 2, SCALE), INV, RZ_SELF, RZ),
    ("turned_with_input_resize", "three", ent("run_video", PTR, 1, Y, F709, PH, PW, 2, 0.0), INV, RZ_YUV, RZ),
    ("input_resize_before_size", "three", ent("run_video", PTR, 1, Y, F709, PH + 2, PW, 2, 0.0), INV, RZ_YUV, RZ),
    ("orient_before_plan_first", "bare", ent("run_video", PTR, 1, Y, F709, PH, PW, 8, 0.0), INV, ORIENT, None),
    ("planes_before_size", "one", ent("run_video", PTR, 1, Y, F709, PH + 2, PW, 2, 0.0), INV, YUV_PLANES, None),
    ("planes_before_scale_tables", "one", ent("run_video", PTR, 1, YS, F709, SH, SW, 2, 0.75), INV, YUV_PLANES, None),
] + [("format_%d" % i, "three", ent("pyramid_video", PTR, 1, Y, fmt(*f), 0, 0, 0, 0.0), INV, why, None) for i, (f, why) in enumerate(BAD_FORMATS)] + [
    ("format_before_null", "three", ent("pyramid_video", None, 1, Y, fmt(7), 0, 0, 0, 0.0), INV, "bits must be 8 .. 16", None),
    ("format_before_scale", "three", ent("pyramid_video", PTR, 1, Y, fmt(8, 0, 3), 0, 0, 0, NAN), INV, "unknown matrix (ACF_HIP_YUV_MATRIX_*)", None),
    ("format_before_plan_first", "bare", ent("pyramid_video", PTR, 1, Y, fmt(17), 0, 0, 0, 0.0), INV, "bits must be 8 .. 16", None),
])
fam("video_bt709", "run_video", [("run_format", "three", ent("run_video", PTR, 1, Y, fmt(16, 1), 0, 0, 0, 0.0), INV, "shift must be 0 for 8 bits, and shift + bits <= 16", None)])
fam("video_10_bits", "pyramid_video", [
    ("odd_base", "three", ent("run_video", ODD, 1, Y10, F10, 0, 0, 0, 0.0), INV, "16-bit samples need an even base", None),
    ("odd_offset", "three", ent("run_video", PTR, 1, ydesc("yuv10", y_offset=1), F10, 0, 0, 0, 0.0), INV, EVEN, None),
    ("odd_stride_row", "three", ent("run_video", PTR, 1, ydesc("yuv10", u_stride_row=2 * PW + 1), F10, 0, 0, 0, 0.0), INV, EVEN, None),
    ("odd_stride_n", "three", ent("pyramid_video", PTR, 1, ydesc("yuv10", v_stride_n=lambda k: k.fb10 + 1), F10, PH, PW, 0, 0.0), INV, EVEN, None),
    ("odd_stride_px", "three", ent("run_video", PTR, 1, ydesc("yuv10", u_stride_px=3), F10, 0, 0, 0, 0.0), INV, EVEN, None),
    ("turned", "turn", ent("pyramid_video", PTR, 1, Y10, F10, PH, PW, 1, 0.0), UNS, WIDE, None),
    ("turned_half", "three", ent("pyramid_video", PTR, 1, Y10, F10, PH, PW, 2, 0.0), UNS, WIDE, None),
    ("reduced", "three", ent("pyramid_video", PTR, 1, Y10, F10, SH, SW, 0, SCALE), UNS, WIDE, None),
    ("orient_below", "three", ent("pyramid_video", PTR, 1, Y10, F10, PH, PW, -1, 0.0), UNS, WIDE, None),
    ("orient_above", "three", ent("pyramid_video", PTR, 1, Y10, F10, PH, PW, 8, 0.0), UNS, WIDE, None),
    ("other_plan", "three", ent("pyramid_video", PTR, 1, Y10, F10, SH, SW, 0, 0.75), UNS, WIDE, None),
    ("turned_before_the_size", "three", ent("pyramid_video", PTR, 1, Y10, F10, 0, PW, 2, 0.0), UNS, WIDE, None),
    ("turned_before_plan_first", "bare", ent("pyramid_video", PTR, 1, Y10, F10, PH, PW, 2, 0.0), UNS, WIDE, None),
    ("scale_before_turned", "three", ent("pyramid_video", PTR, 1, Y10, F10, PH, PW, 1, NAN), INV, VSCALE, None),
    ("planes_before_even", "one", ent("run_video", PTR, 1, ydesc("yuv10", y_offset=1), F10, 0, 0, 0, 0.0), INV, YUV_PLANES, None),
    ("description_before_even", "three", ent("run_video", PTR, 1, ydesc("yuv10", y_offset=1, sub_x=2), F10, 0, 0, 0, 0.0), INV, "sub_x and sub_y must be 0 or 1", None),
    ("even_before_input_resize", "three", ent("run_video", PTR, 1, ydesc("yuv10", y_offset=1), F10, 0, 0, 0, 0.0), INV, EVEN, RZ),
])
fam("video_default_format", None, [   # (the default format is the YUV entry of the call's family)
    ("orient_above", "three", ent("run_video", PTR, 1, Y, None, PH, PW, 8, 0.0), INV, ORIENT, None),
    ("size", "three", ent("run_video", PTR, 1, Y, None, PH + 2, PW, 0, 0.0), INV, UPRIGHT, None),
    ("one_plane", "one", ent("run_video", PTR, 1, Y, None, 0, 0, 0, 0.0), INV, YUV_PLANES, None),
    ("reduced_nan_scale", "three", ent("pyramid_video", PTR, 1, YS, None, SH, SW, 0, NAN), INV, VSCALE, None),
    ("other_plan", "three", ent("run_video", PTR, 1, YS, None, SH, SW, 2, 0.75), INV, REDUCED, None),
])


def opens(tag, who, o, D, DV, fbytes, rows, cols, resized):
    """The rows the three stream_open calls of these families share.  o(desc, frame_bytes, rows, cols, orient, cap, depth): the call;
    D / DV: the description and its name in the contexts; rows x cols: the frames."""
    size_text = REDUCED if resized else UPRIGHT
    fam(tag, who, [
        ("null_description", "three", o(None, fbytes, rows, cols, 2, 64, 2), INV, "null description", None),
        ("orient_below", "three", o(D, fbytes, rows, cols, -1, 64, 2), INV, ORIENT, None),
        ("orient_above", "three", o(D, fbytes, rows, cols, 8, 64, 2), INV, ORIENT, None),
        ("no_rows", "three", o(D, fbytes, 0, cols, 2, 64, 2), INV, ORIENT, None),
        ("negative_cols", "three", o(D, fbytes, rows, -1, 2, 64, 2), INV, ORIENT, None),
        ("size_code_1", "three", o(D, fbytes, rows, cols, 1, 64, 2), INV, size_text, None),
        ("size_code_2", "three", o(D, fbytes, rows + 2, cols, 2, 64, 2), INV, size_text, None),
        ("size_code_1_quarter_turn", "turn", o(D, fbytes, rows, cols + 2, 1, 64, 2), INV, size_text, None),
        ("one_plane", "one", o(D, fbytes, rows, cols, 2, 64, 2), INV, OPEN_PLANES, None),
        ("five_planes", "five", o(D, fbytes, rows, cols, 2, 64, 2), INV, OPEN_PLANES, None),
        ("with_input_resize", "three", o(D, fbytes, rows, cols, 2, 64, 2), INV, OPEN_PLANES, RZ),
        ("streams", "multi", o(D, fbytes, rows, cols, 2, 64, 2), UNS, STREAMS, None),
        ("no_plan", "bare", o(D, fbytes, rows, cols, 2, 64, 2), NOPLAN, "plan first", None),
        ("depth", "three", o(D, fbytes, rows, cols, 2, 64, 9), INV, DEPTH, None),
        ("cap", "three", o(D, fbytes, rows, cols, 2, 0, 2), INV, DEPTH, None),
        ("plane_outside", "three", o(D, lambda k: fbytes(k) - 1, rows, cols, 2, 64, 2), INV, INSIDE, None),
        ("plane_below", "three", o(ydesc(DV, v_offset=-8), fbytes, rows, cols, 2, 64, 2), INV, INSIDE, None),
        ("stride_n", "three", o(ydesc(DV, y_stride_n=lambda k: fbytes(k) + 4), fbytes, rows, cols, 2, 64, 2), INV, STRIDE_N, None),
        ("plan_first_before_orient", "bare", o(D, fbytes, rows, cols, 8, 64, 2), NOPLAN, "plan first", None),
        ("streams_before_depth", "multi", o(D, fbytes, rows, cols, 2, 64, 9), UNS, STREAMS, None),
        ("depth_before_description", "three", o(ydesc(DV, sub_x=2), fbytes, rows, cols, 2, 0, 2), INV, DEPTH, None),
        ("description_before_planes", "five", o(ydesc(DV, sub_x=2), fbytes, rows, cols, 2, 64, 2), INV, "sub_x and sub_y must be 0 or 1", None),
        ("planes_before_extent", "one", o(D, lambda k: fbytes(k) - 1, rows, cols, 2, 64, 2), INV, OPEN_PLANES, None),
        ("extent_before_stride_n", "three", o(ydesc(DV, u_stride_n=lambda k: fbytes(k) + 4, v_offset=fbytes), fbytes, rows, cols, 2, 64, 2), INV, INSIDE, None),
    ])


o_oriented = lambda d, fb, r, c, o, cap, depth: ent("stream_open_yuv_oriented", d, fb, r, c, o, cap, depth)
o_oriented_resized = lambda d, fb, r, c, o, cap, depth, s=SCALE: ent("stream_open_yuv_oriented_resized", d, fb, r, c, o, s, cap, depth)
o_video = lambda d, fb, r, c, o, cap, depth, f=F709, s=0.0: ent("stream_open_video", d, f, fb, r, c, o, s, cap, depth)
o_video_reduced = lambda d, fb, r, c, o, cap, depth: o_video(d, fb, r, c, o, cap, depth, F709, SCALE)
opens("stream_open_yuv_oriented", "stream_open_yuv_oriented", o_oriented, Y, "yuv", FB, PH, PW, False)
opens("stream_open_yuv_oriented_resized", "stream_open_yuv_oriented_resized", o_oriented_resized, YS, "yuvS", FBS, SH, SW, True)
opens("stream_open_video_bt709", "stream_open_video", o_video, Y, "yuv", FB, PH, PW, False)
opens("stream_open_video_bt709_reduced", "stream_open_video", o_video_reduced, YS, "yuvS", FBS, SH, SW, True)
W_O, W_OR, W_V = "stream_open_yuv_oriented", "stream_open_yuv_oriented_resized", "stream_open_video"
fam(W_O, W_O, [
    ("size_code_0", "three", o_oriented(Y, FB, PH + 2, PW, 0, 64, 2), INV, UPRIGHT, None),
    ("orient_before_streams", "multi", o_oriented(Y, FB, PH, PW, 8, 64, 2), INV, ORIENT, None),
    ("size_before_streams", "multi", o_oriented(Y, FB, PH + 2, PW, 2, 64, 2), INV, UPRIGHT, None),
    ("size_before_depth", "three", o_oriented(Y, FB, PH + 2, PW, 2, 64, 9), INV, UPRIGHT, None),
])
fam(W_OR, W_OR, [
    ("nan_scale", "three", o_oriented_resized(YS, FBS, SH, SW, 2, 64, 2, NAN), INV, SIZE_SCALE, None),
    ("negative_scale", "three", o_oriented_resized(YS, FBS, SH, SW, 2, 64, 2, -0.5), INV, SIZE_SCALE, None),
    ("zero_scale", "three", o_oriented_resized(YS, FBS, SH, SW, 2, 64, 2, 0.0), INV, SIZE_SCALE, None),
    ("other_plan", "three", o_oriented_resized(YS, FBS, SH, SW, 2, 64, 2, 0.75), INV, REDUCED, None),
    ("orient_before_streams", "multi", o_oriented_resized(YS, FBS, SH, SW, 8, 64, 2), INV, ORIENT, None),
    ("planes_before_scale", "one", o_oriented_resized(YS, FBS, SH, SW, 2, 64, 2, NAN), INV, OPEN_PLANES, None),
    ("plan_before_the_extent", "three", o_oriented_resized(YS, lambda k: k.fbS - 1, SH + 2, SW, 2, 64, 2), INV, REDUCED, None),
    ("room_for_the_plan_size_only", "three",
     o_oriented_resized(ydesc("yuvS", y_stride_n=FB, u_stride_n=FB, v_stride_n=FB), FB, SH, SW, 2, 64, 2), INV, INSIDE, None),
])
fam(W_OR + "_code_0", None, [   # (code 0 is stream_open_yuv_resized)
    ("size", "three", o_oriented_resized(YS, FBS, SH + 2, SW, 0, 64, 2), INV, REDUCED, None),
    ("nan_scale", "three", o_oriented_resized(YS, FBS, SH, SW, 0, 64, 2, NAN), INV, SIZE_SCALE, None),
    ("one_plane", "one", o_oriented_resized(YS, FBS, SH, SW, 0, 64, 2), INV, OPEN_PLANES, None),
    ("plane_outside", "three", o_oriented_resized(YS, lambda k: k.fbS - 1, SH, SW, 0, 64, 2), INV, INSIDE, None),
])
fam(W_V + "_bt709", W_V, [
    ("null_description_plain", "three", o_video(None, FB, 0, 0, 0, 64, 2), INV, "null description", None),
    ("size_code_0", "three", o_video(Y, FB, PH + 2, PW, 0, 64, 2), INV, UPRIGHT, None),
    ("nan_scale", "three", o_video(YS, FBS, SH, SW, 0, 64, 2, F709, NAN), INV, VSCALE, None),
    ("negative_scale", "three", o_video(YS, FBS, SH, SW, 0, 64, 2, F709, -0.5), INV, VSCALE, None),
    ("other_plan", "three", o_video(YS, FBS, SH, SW, 0, 64, 2, F709, 0.75), INV, REDUCED, None),
    ("plain_one_plane", "one", o_video(Y, FB, 0, 0, 0, 64, 2), INV, OPEN_PLANES, None),
    ("plain_streams", "multi", o_video(Y, FB, 0, 0, 0, 64, 2), UNS, STREAMS, None),
    ("plain_plane_outside", "three", o_video(Y, lambda k: k.fb - 1, 0, 0, 0, 64, 2), INV, INSIDE, None),
    ("plain_stride_n", "three", o_video(ydesc("yuv", v_stride_n=lambda k: k.fb + 4), FB, 0, 0, 0, 64, 2), INV, STRIDE_N, None),
    ("plan_first_before_format", "bare", o_video(Y, FB, 0, 0, 0, 64, 2, fmt(7)), NOPLAN, "plan first", None),
    ("format_before_scale", "three", o_video(Y, FB, 0, 0, 0, 64, 2, fmt(8, 0, 0, 2), NAN), INV, "full_range must be 0 or 1", None),
    ("format_before_streams", "multi", o_video(Y, FB, 0, 0, 0, 64, 2, fmt(17)), INV, "bits must be 8 .. 16", None),
    ("scale_before_streams", "multi", o_video(Y, FB, 0, 0, 0, 64, 2, F709, NAN), INV, VSCALE, None),
    ("scale_before_orient", "three", o_video(Y, FB, PH, PW, 8, 64, 2, F709, -1.0), INV, VSCALE, None),
    ("size_before_depth", "three", o_video(Y, FB, PH + 2, PW, 2, 64, 9), INV, UPRIGHT, None),
    ("planes_before_scale_tables", "one", o_video(YS, FBS, SH, SW, 2, 64, 2, F709, 0.75), INV, OPEN_PLANES, None),
    ("streams_before_orient", "multi", o_video(Y, FB, PH, PW, 8, 64, 2), UNS, STREAMS, None),
    ("streams_before_orient_below", "multi", o_video(Y, FB, PH, PW, -1, 64, 2), UNS, STREAMS, None),
    ("streams_before_no_rows", "multi", o_video(Y, FB, 0, PW, 2, 64, 2), UNS, STREAMS, None),
    ("streams_before_size", "multi", o_video(Y, FB, PH + 2, PW, 2, 64, 2), UNS, STREAMS, None),
    ("streams_before_size_code_0", "multi", o_video(Y, FB, PH + 2, PW, 0, 64, 2), UNS, STREAMS, None),
    ("streams_before_orient_reduced", "multi", o_video(YS, FBS, SH, SW, 8, 64, 2, F709, SCALE), UNS, STREAMS, None),
] + [("format_%d" % i, "three", o_video(Y, FB, 0, 0, 0, 64, 2, fmt(*f)), INV, why, None) for i, (f, why) in enumerate(BAD_FORMATS)])
fam(W_V + "_10_bits", W_V, [
    ("null_description", "three", o_video(None, FB10, 0, 0, 0, 64, 2, F10), INV, "null description", None),
    ("no_rows", "three", o_video(Y10, FB10, 0, PW, 0, 64, 2, F10), INV, ORIENT, None),
    ("negative_cols", "three", o_video(Y10, FB10, PH, -1, 0, 64, 2, F10), INV, ORIENT, None),
    ("size_code_0", "three", o_video(Y10, FB10, PH + 2, PW, 0, 64, 2, F10), INV, UPRIGHT, None),
    ("nan_scale", "three", o_video(Y10, FB10, 0, 0, 0, 64, 2, F10, NAN), INV, VSCALE, None),
    ("one_plane", "one", o_video(Y10, FB10, 0, 0, 0, 64, 2, F10), INV, OPEN_PLANES, None),
    ("five_planes", "five", o_video(Y10, FB10, 0, 0, 0, 64, 2, F10), INV, OPEN_PLANES, None),
    ("with_input_resize", "three", o_video(Y10, FB10, 0, 0, 0, 64, 2, F10), INV, OPEN_PLANES, RZ),
    ("streams", "multi", o_video(Y10, FB10, 0, 0, 0, 64, 2, F10), UNS, STREAMS, None),
    ("no_plan", "bare", o_video(Y10, FB10, 0, 0, 0, 64, 2, F10), NOPLAN, "plan first", None),
    ("depth", "three", o_video(Y10, FB10, 0, 0, 0, 64, 1, F10), INV, DEPTH, None),
    ("odd_offset", "three", o_video(ydesc("yuv10", y_offset=1), FB10, 0, 0, 0, 64, 2, F10), INV, EVEN, None),
    ("odd_stride_row", "three", o_video(ydesc("yuv10", u_stride_row=2 * PW + 1), FB10, 0, 0, 0, 64, 2, F10), INV, EVEN, None),
    ("odd_stride_n", "three", o_video(ydesc("yuv10", v_stride_n=lambda k: k.fb10 + 1), FB10, 0, 0, 0, 64, 2, F10), INV, EVEN, None),
    ("turned", "turn", o_video(Y10, FB10, PH, PW, 1, 64, 2, F10), UNS, WIDE, None),
    ("turned_half", "three", o_video(Y10, FB10, PH, PW, 2, 64, 2, F10), UNS, WIDE, None),
    ("reduced", "three", o_video(Y10, FB10, SH, SW, 0, 64, 2, F10, SCALE), UNS, WIDE, None),
    ("orient_below", "three", o_video(Y10, FB10, PH, PW, -1, 64, 2, F10), INV, ORIENT, None),
    ("orient_above", "three", o_video(Y10, FB10, PH, PW, 8, 64, 2, F10), INV, ORIENT, None),
    ("orient_before_reduced", "three", o_video(Y10, FB10, SH, SW, 8, 64, 2, F10, SCALE), INV, ORIENT, None),
    ("no_rows_before_turned", "three", o_video(Y10, FB10, 0, PW, 2, 64, 2, F10), INV, ORIENT, None),
    ("streams_before_orient", "multi", o_video(Y10, FB10, PH, PW, 8, 64, 2, F10), UNS, STREAMS, None),
    ("streams_before_turned", "multi", o_video(Y10, FB10, PH, PW, 2, 64, 2, F10), UNS, STREAMS, None),
    ("last_word_high_byte_outside", "three", o_video(Y10, lambda k: k.fb10 - 1, 0, 0, 0, 64, 2, F10), INV, INSIDE, None),
    ("last_word_outside", "three", o_video(Y10, lambda k: k.fb10 - 2, 0, 0, 0, 64, 2, F10), INV, INSIDE, None),
    ("stride_n", "three", o_video(ydesc("yuv10", y_stride_n=lambda k: k.fb10 + 4), FB10, 0, 0, 0, 64, 2, F10), INV, STRIDE_N, None),
    ("scale_before_turned", "three", o_video(Y10, FB10, PH, PW, 1, 64, 2, F10, NAN), INV, VSCALE, None),
    ("description_before_planes", "five", o_video(ydesc("yuv10", sub_y=2), FB10, 0, 0, 0, 64, 2, F10), INV, "sub_x and sub_y must be 0 or 1", None),
    ("extent_before_stride_n", "three", o_video(ydesc("yuv10", u_stride_n=lambda k: k.fb10 + 4), lambda k: k.fb10 - 1, 0, 0, 0, 64, 2, F10), INV, INSIDE, None),
])
fam(W_V + "_default_format", None, [   # (the default format is the open call of the family)
    ("orient_above", "three", o_video(Y, FB, PH, PW, 8, 64, 2, None), INV, ORIENT, None),
    ("size", "three", o_video(Y, FB, PH + 2, PW, 0, 64, 2, None), INV, UPRIGHT, None),
    ("one_plane", "one", o_video(Y, FB, 0, 0, 0, 64, 2, None), INV, OPEN_PLANES, None),
    ("plane_outside", "three", o_video(Y, lambda k: k.fb - 1, 0, 0, 0, 64, 2, None), INV, INSIDE, None),
    ("reduced_other_plan", "three", o_video(YS, FBS, SH, SW, 2, 64, 2, None, 0.75), INV, REDUCED, None),
    ("orient_before_streams", "multi", o_video(Y, FB, PH, PW, 8, 64, 2, None), INV, ORIENT, None),
    ("size_before_streams", "multi", o_video(Y, FB, PH + 2, PW, 2, 64, 2, None), INV, UPRIGHT, None),
])
ROWS += FAMILY_ROWS

IDS = [r[0] for r in ROWS]
assert len(set(IDS)) == len(IDS)


@pytest.fixture(scope="module")
def ctxs():
    k = Ctxs()
    yield k
    k.close()


def test_every_context_takes_its_good_call(ctxs):
    for name in ("three", "one", "five", "odd", "multi", "turn"):
        ctxs.good(name, getattr(ctxs, name))
    d = ctxs.three
    d.run_yuv_resized(ctxs.x, 2, ctxs.yuvS, SH, SW, SCALE)
    d.run_image_resized(ctxs.ptr, 2, ctxs.imgS, SH, SW, SCALE)
    d.run_yuv(ctxs.x, 2, ctxs.yuv)
    d.run_image(ctxs.ptr, 2, ctxs.img)
    for opener in (lambda: d.stream_open(capi.PIX_RGB, 0, 64, 2), lambda: d.stream_open_yuv(ctxs.yuv, ctxs.fb, 64, 2),
                   lambda: d.stream_open_yuv_resized(ctxs.yuvS, ctxs.fbS, SH, SW, SCALE, 64, 2)):
        opener()
        d.stream_close()


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_refused_with_its_code_and_message(ctxs, row):
    from acf_amd.detector import HipError
    rid, name, call, code, piece, around = row
    det = ctxs.bare() if name == "bare" else getattr(ctxs, name)
    if around:
        around[0](ctxs, det)
    try:
        with pytest.raises(HipError) as e:
            call(ctxs, det)
        assert e.value.code == code, e.value
        assert piece in str(e.value), e.value
        if name == "bare":
            det.plan(PH, PW, 3, 2)
        if around and around[0] is rz_on:
            det.run_u8(ctxs.x, capi.PIX_GRAY if name == "one" else capi.PIX_RGB, 0, n=2)   # (unreduced frames while the resize is on)
            det.synchronize()
    finally:
        if around:
            around[1](ctxs, det)
    ctxs.good(name, det)
    if name == "bare":
        det.close()
