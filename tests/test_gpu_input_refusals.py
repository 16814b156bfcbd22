"""What the input entries refuse, entry by entry: the 8-bit, tensor and YUV entries, their resized forms, the three stream_open calls
and the settings in front of them (set_input_resize, set_yuv_layout, yuv_to_rgb8).

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
    """The contexts of the table, made once: three-plane, one-plane, five-plane, an odd-sized plan, sub-batch streams."""

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
        self.yuv, self.fb = HipDetector.yuv_desc("i420", PH, PW)
        self.yuvS, self.fbS = HipDetector.yuv_desc("i420", SH, SW)
        self.img = capi.ImageDesc(capi.T_U8, 3, 3 * PH * PW, PH * PW, PW, 1)
        self.imgS = capi.ImageDesc(capi.T_U8, 3, 3 * SH * SW, SH * SW, SW, 1)

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
        for d in (self.three, self.one, self.five, self.odd, self.multi):
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
IDS = [r[0] for r in ROWS]
assert len(set(IDS)) == len(IDS)


@pytest.fixture(scope="module")
def ctxs():
    k = Ctxs()
    yield k
    k.close()


def test_every_context_takes_its_good_call(ctxs):
    for name in ("three", "one", "five", "odd", "multi"):
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
