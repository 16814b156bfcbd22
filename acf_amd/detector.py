"""Thin Python handle on the C ABI (include/acf_hip.h) for tests and bench.py.

Every method is a direct call into libacf_hip.so; there is no Python or CPU
implementation behind it.  Frames are float32 [n][d][W][H] (H contiguous, the
reference's transposed planar layout, MatP.cpp:51-73) either as a torch CUDA
tensor / raw device pointer (run, pyramid) or as a numpy array (run_host).
"""
import ctypes as C

import numpy as np

from . import capi


class HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("acf_hip error %d: %s" % (code, msg))
        self.code = code


def _dev_ptr(x):
    if isinstance(x, int):
        return x
    # torch tensor
    assert x.is_cuda and x.is_contiguous() and x.dtype.is_floating_point and x.element_size() == 4
    return x.data_ptr()


def _dev_ptr_u8(x):
    if isinstance(x, int):
        return x
    assert x.is_cuda and x.is_contiguous() and x.element_size() == 1
    return x.data_ptr()


class PinnedBuffer:
    """Page-locked host memory from the library (acf_hip_host_alloc), viewed as a numpy uint8 array."""

    def __init__(self, nbytes):
        self.lib = capi.load()
        self.ptr = C.c_void_p()
        if self.lib.acf_hip_host_alloc(nbytes, C.byref(self.ptr)):
            raise HipError(5, "acf_hip_host_alloc failed")
        self.array = np.ctypeslib.as_array(C.cast(self.ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def close(self):
        if self.ptr:
            self.array = None
            self.lib.acf_hip_host_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipDetector:
    def __init__(self, model=None, H=0, W=0, d_in=3, max_batch=1, max_hits=4096, device=0, stream=None, taps=False, streams=1):
        self.lib = capi.load()
        self.ctx = C.c_void_p()
        rc = self.lib.acf_hip_create(device, C.c_void_p(stream or 0), C.byref(self.ctx))
        if rc:
            raise HipError(rc, "acf_hip_create failed (no gfx950 device?)")
        self._keep = None
        self.levels = []
        self.nChns = 0
        if taps:
            self._chk(self.lib.acf_hip_set_option(self.ctx, b"taps", 1))
        if streams > 1:
            # sub-batch contexts on their own streams (takes effect at plan time)
            self._chk(self.lib.acf_hip_set_option(self.ctx, b"streams", streams))
        if model is not None:
            self.set_model(model)
            if H and W:
                self.plan(H, W, d_in, max_batch, max_hits)

    def _chk(self, rc):
        if rc:
            raise HipError(rc, (self.lib.acf_hip_last_error(self.ctx) or b"").decode())

    def close(self):
        if self.ctx:
            self.lib.acf_hip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_model(self, model):
        self.model = model
        self.params, self._keep = capi.make_params(model)
        self._chk(self.lib.acf_hip_set_model(self.ctx, C.byref(self.params)))

    def plan(self, H, W, d_in=3, max_batch=1, max_hits=4096):
        self._chk(self.lib.acf_hip_plan(self.ctx, H, W, d_in, max_batch, max_hits))
        self.H, self.W, self.d_in, self.max_batch, self.max_hits = H, W, d_in, max_batch, max_hits
        n, nc = C.c_int(), C.c_int()
        self._chk(self.lib.acf_hip_num_levels(self.ctx, C.byref(n), C.byref(nc)))
        lv = (capi.Level * n.value)()
        self._chk(self.lib.acf_hip_get_levels(self.ctx, lv, n.value))
        self.levels = list(lv)
        self.nChns = nc.value
        tot = C.c_int64()
        self._chk(self.lib.acf_hip_pyramid_floats(self.ctx, C.byref(tot)))
        self.pyr_floats = tot.value
        self.ldcf_levels = []
        if int(self.params.ldcfK) > 0:
            ll = (capi.Level * n.value)()
            self._chk(self.lib.acf_hip_get_ldcf_levels(self.ctx, ll, n.value))
            self.ldcf_levels = list(ll)

    # ---- hot path
    def pyramid(self, frames, n=None):
        n = n if n is not None else frames.shape[0]
        self._chk(self.lib.acf_hip_pyramid(self.ctx, C.c_void_p(_dev_ptr(frames)), n))

    def detect(self):
        self._chk(self.lib.acf_hip_detect(self.ctx))

    def run(self, frames, n=None):
        n = n if n is not None else frames.shape[0]
        self._chk(self.lib.acf_hip_run(self.ctx, C.c_void_p(_dev_ptr(frames)), n))

    def run_host(self, frames):
        frames = np.ascontiguousarray(frames, dtype=np.float32)
        self._chk(self.lib.acf_hip_run_host(self.ctx, capi.fptr(frames), frames.shape[0]))

    def pyramid_u8(self, frames, pix=capi.PIX_RGB, row_stride=0, n=None):
        """frames: torch uint8 CUDA tensor [n][H][W][cpp] (upright, packed; PIX_NV12 / PIX_NV21: [n][frame bytes], see
        u8_frame_bytes and set_yuv_layout) or a raw device pointer."""
        n = n if n is not None else frames.shape[0]
        self._chk(self.lib.acf_hip_pyramid_u8(self.ctx, C.c_void_p(_dev_ptr_u8(frames)), n, pix, row_stride))

    def run_u8(self, frames, pix=capi.PIX_RGB, row_stride=0, n=None):
        n = n if n is not None else frames.shape[0]
        self._chk(self.lib.acf_hip_run_u8(self.ctx, C.c_void_p(_dev_ptr_u8(frames)), n, pix, row_stride))

    # ---- upright device tensors of any strides: uint8 / float16 / bfloat16 / float32 (acf_hip_pyramid_image / run_image)
    @staticmethod
    def _torch_dtype_code(t):
        import torch
        codes = {torch.uint8: capi.T_U8, torch.float16: capi.T_F16, torch.bfloat16: capi.T_BF16, torch.float32: capi.T_F32}
        if t.dtype not in codes:
            raise HipError(capi.E_INVALID, "tensor entry: dtype must be uint8, float16, bfloat16 or float32, not %s" % t.dtype)
        return codes[t.dtype]

    def _image_of(self, t, layout, scale=None, orient=0):
        """(device pointer, n, capi.ImageDesc) of a device tensor [n, c, H, W] (layout "nchw") or [n, H, W, c] ("nhwc", taken as the
        permuted view); the strides are the tensor's own: nothing is copied or made contiguous.  scale: the resized entries — the
        tensor is the unreduced frame, the plan is for resize_dims of its size.  orient: the oriented entries — the tensor is the
        frame as stored, the plan is for oriented_dims of its size."""
        if layout not in ("nchw", "nhwc"):
            raise HipError(capi.E_INVALID, "tensor entry: layout must be \"nchw\" or \"nhwc\"")
        if t.dim() != 4 or not t.is_cuda:
            raise HipError(capi.E_INVALID, "tensor entry: a device tensor of four dimensions")
        if layout == "nhwc":
            t = t.permute(0, 3, 1, 2)
        n, ch, h, w = t.shape
        if scale is not None:
            if self._torch_dtype_code(t) != capi.T_U8:
                raise HipError(capi.E_UNSUPPORTED, "resized tensor entry: uint8 only, not %s" % t.dtype)
            if ch != self.d_in:
                raise HipError(capi.E_INVALID, "resized tensor entry: the tensor has c = %d, the plan %d" % (ch, self.d_in))
        elif orient:
            if ch != self.d_in:
                raise HipError(capi.E_INVALID, "oriented tensor entry: the tensor has c = %d, the plan %d" % (ch, self.d_in))
        elif (h, w, ch) != (self.H, self.W, self.d_in):
            raise HipError(capi.E_INVALID, "tensor entry: the tensor is c = %d, H = %d, W = %d; the plan is for %d, %d, %d" % (ch, h, w, self.d_in, self.H, self.W))
        sn, sc, sy, sx = t.stride()
        return t.data_ptr(), n, capi.ImageDesc(self._torch_dtype_code(t), ch, sn, sc, sy, sx)

    def _entry_for(self, src_rows, src_cols, orient, scale):
        """(name suffix, further arguments) of the most specific entry for what the caller states about the frames — a size, an
        orientation, a scale — pyramid, run and stream_open alike; the library takes all of them through one general entry.  Code 0
        beside a scale is the resized entry, beside a size alone the oriented one."""
        if scale is not None and not orient:
            return "_resized", (src_rows, src_cols, float(scale))
        if scale is not None:
            return "_oriented_resized", (src_rows, src_cols, orient, float(scale))
        if orient or src_rows is not None:
            return "_oriented", (*self._src_size(orient, src_rows, src_cols), orient)
        return "", ()

    def _source_call(self, stem, ptr, n, desc, src_rows=None, src_cols=None, orient=0, scale=None):
        suffix, args = self._entry_for(src_rows, src_cols, orient, scale)
        self._chk(getattr(self.lib, "acf_hip_" + stem + suffix)(self.ctx, ptr, n, C.byref(desc), *args))

    def _image_call(self, run, ptr, n, desc, *geometry):
        self._source_call("run_image" if run else "pyramid_image", C.c_void_p(ptr), n, desc, *geometry)

    def _yuv_call(self, run, base, n, desc, *geometry):
        self._source_call("run_yuv" if run else "pyramid_yuv", C.c_void_p(base if isinstance(base, int) else base.data_ptr()), n, desc, *geometry)

    def _tensor_call(self, run, t, layout, orient, scale=None):
        ptr, n, desc = self._image_of(t, layout, scale, orient)
        rows, cols = (t.shape[2], t.shape[3]) if layout == "nchw" else (t.shape[1], t.shape[2])
        own = orient or scale is not None   # (else the plan's size, which _image_of has held the tensor against: the plain entry)
        self._image_call(run, ptr, n, desc, rows if own else None, cols if own else None, orient, scale)

    def pyramid_tensor(self, t, layout="nchw", orient=0):
        """t: device tensor [n, c, H, W] of any strides (or [n, H, W, c] with layout="nhwc"), uint8 / float16 / bfloat16 / float32.
        orient (capi.ORIENT_*, rot + 4 * mirror): t is the frame as stored, [n, c, Hs, Ws]; the plan is for oriented_dims(Hs, Ws, orient)
        and detections are in the upright frame (unorient_boxes maps them back).  0 takes the un-oriented entry."""
        self._tensor_call(False, t, layout, orient)

    def run_tensor(self, t, layout="nchw", orient=0):
        self._tensor_call(True, t, layout, orient)

    def pyramid_image_oriented(self, ptr, n, desc, src_rows, src_cols, orient):
        """The raw oriented entry: desc describes frames of src_rows x src_cols; the plan is for oriented_dims of them."""
        self._image_call(False, ptr, n, desc, src_rows, src_cols, orient)

    def run_image_oriented(self, ptr, n, desc, src_rows, src_cols, orient):
        self._image_call(True, ptr, n, desc, src_rows, src_cols, orient)

    def pyramid_tensor_resized(self, t, scale, layout="nchw", orient=0):
        """t: uint8 device tensor of the UNREDUCED frames [n, c, rows, cols] of any strides; the plan is for resize_dims(rows, cols,
        scale).  The apps' resize and the ingest in one kernel; detections are in the reduced frame (unscale_boxes maps them back).
        orient (capi.ORIENT_*): t is the unreduced frame AS STORED; it is turned upright, then reduced: the plan is for
        oriented_resized_dims(rows, cols, orient, scale), and unscale_boxes, then unorient_boxes map detections back."""
        self._tensor_call(False, t, layout, orient, scale)

    def run_tensor_resized(self, t, scale, layout="nchw", orient=0):
        self._tensor_call(True, t, layout, orient, scale)

    def pyramid_image(self, ptr, n, desc):
        """The raw entry: a device pointer (int) and a capi.ImageDesc."""
        self._image_call(False, ptr, n, desc)

    def run_image(self, ptr, n, desc):
        self._image_call(True, ptr, n, desc)

    def pyramid_image_resized(self, ptr, n, desc, src_rows, src_cols, scale, orient=0):
        """The raw resized entry: desc (uint8) describes frames of src_rows x src_cols; the plan is for resize_dims of them — with
        orient, for oriented_resized_dims (the frame is turned upright first, then reduced)."""
        self._image_call(False, ptr, n, desc, src_rows, src_cols, orient, scale)

    def run_image_resized(self, ptr, n, desc, src_rows, src_cols, scale, orient=0):
        self._image_call(True, ptr, n, desc, src_rows, src_cols, orient, scale)

    @staticmethod
    def image_extent(desc, h, w, n):
        """(lowest, highest) element offset from the frames pointer that a call with this capi.ImageDesc reads (host arithmetic)."""
        lo, hi = C.c_int64(), C.c_int64()
        rc = capi.load().acf_hip_image_extent(C.byref(desc), h, w, n, C.byref(lo), C.byref(hi))
        if rc:
            raise HipError(rc, "acf_hip_image_extent")
        return lo.value, hi.value

    # ---- YUV 4:2:0 video frames (PIX_NV12 / PIX_NV21) in the 8-bit entries
    @staticmethod
    def u8_frame_bytes(pix, rows, cols, row_stride=0):
        """Bytes from one tight frame of layout `pix` to the next (host arithmetic: no context, no GPU)."""
        out = C.c_int64()
        rc = capi.load().acf_hip_u8_frame_bytes(pix, rows, cols, row_stride, C.byref(out))
        if rc:
            raise HipError(rc, "acf_hip_u8_frame_bytes(pix=%d, %d x %d, stride %d)" % (pix, rows, cols, row_stride))
        return out.value

    def set_yuv_layout(self, chroma_offset=0, frame_stride=0):
        """Where an NV12 / NV21 frame's chroma plane starts and how far frames are apart, in bytes (0, 0 = tight); until the next plan."""
        self._chk(self.lib.acf_hip_set_yuv_layout(self.ctx, chroma_offset, frame_stride))

    def yuv420_to_rgb(self, frame, rows, cols, pix=capi.PIX_NV12, row_stride=0, chroma_offset=0):
        """frame: the bytes of one NV12 / NV21 frame (host, uint8) -> uint8 [rows][cols][3] R, G, B (cvtColor COLOR_YUV2RGB_NV12 / _NV21)."""
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        stride = row_stride or cols
        if rows > 0 and cols > 0 and frame.size < (chroma_offset or stride * rows) + stride * (rows // 2):
            raise HipError(capi.E_INVALID, "yuv420_to_rgb: frame buffer smaller than the frame")
        out = np.zeros((max(rows, 0), max(cols, 0), 3), dtype=np.uint8)
        self._chk(self.lib.acf_hip_op_yuv420_to_rgb(self.ctx, frame.ctypes.data, rows, cols, pix, row_stride, chroma_offset, out.ctypes.data))
        return out

    # ---- YUV frames of three planes described by offsets and byte strides (acf_hip_pyramid_yuv / run_yuv): I420 / YV12 / I422 /
    # I444, packed 4:2:2, NV12 / NV21, separately allocated planes
    @staticmethod
    def yuv_desc(layout, H, W, row_stride=0):
        """(capi.YuvDesc, frame bytes) of a named layout: capi.YUV_* or its name ("i420", "yuyv", ...); host arithmetic."""
        code = capi.YUV_NAMES.get(layout.lower(), -1) if isinstance(layout, str) else layout
        desc, fb = capi.YuvDesc(), C.c_int64()
        rc = capi.load().acf_hip_yuv_layout(code, H, W, row_stride, C.byref(desc), C.byref(fb))
        if rc:
            raise HipError(rc, "acf_hip_yuv_layout(%r, %d x %d, stride %d)" % (layout, H, W, row_stride))
        return desc, fb.value

    @staticmethod
    def yuv_extent(desc, h, w, n):
        """([first Y, U, V], [last Y, U, V]): the lowest and highest byte offset from the base a call reads of each plane."""
        lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        rc = capi.load().acf_hip_yuv_extent(C.byref(desc), h, w, n, lo, hi)
        if rc:
            raise HipError(rc, "acf_hip_yuv_extent")
        return list(lo), list(hi)

    def pyramid_yuv(self, base, n, desc, orient=0, src_rows=None, src_cols=None):
        """base: a torch uint8 CUDA tensor (its first byte is the base; it need not be contiguous) or a device pointer.
        orient (capi.ORIENT_*): desc describes the frame as stored, src_rows x src_cols; the plan is for oriented_dims of that."""
        self._yuv_call(False, base, n, desc, src_rows, src_cols, orient)

    def run_yuv(self, base, n, desc, orient=0, src_rows=None, src_cols=None):
        self._yuv_call(True, base, n, desc, src_rows, src_cols, orient)

    def _src_size(self, orient, src_rows, src_cols):
        """The stored frame's size where the caller left it out: the plan's, turned back (odd rot swaps rows and columns)."""
        if src_rows is not None and src_cols is not None:
            return src_rows, src_cols
        return (self.W, self.H) if orient & 1 else (self.H, self.W)

    def pyramid_yuv_resized(self, base, n, desc, src_rows, src_cols, scale, orient=0):
        """desc describes frames of src_rows x src_cols; the plan is for resize_dims(src_rows, src_cols, scale).  Conversion, the apps'
        resize and the ingest in one kernel; detections are in the reduced frame (unscale_boxes maps them back).
        orient (capi.ORIENT_*): the frames as stored; turned upright, then reduced: the plan is for oriented_resized_dims(src_rows,
        src_cols, orient, scale); unscale_boxes, then unorient_boxes map detections back."""
        self._yuv_call(False, base, n, desc, src_rows, src_cols, orient, scale)

    def run_yuv_resized(self, base, n, desc, src_rows, src_cols, scale, orient=0):
        self._yuv_call(True, base, n, desc, src_rows, src_cols, orient, scale)

    @staticmethod
    def yuv_planes_desc(y, u, v, sub_x, sub_y):
        """(base pointer, n, capi.YuvDesc) of three torch uint8 device tensors [n, rows, cols] (or [rows, cols]) wherever they lie:
        Y is the base, U and V are described by their distance from it (which may be negative) and their own strides."""
        def plane(t):
            if t.dim() == 2:
                t = t[None]
            if t.dim() != 3 or not t.is_cuda or t.element_size() != 1:
                raise HipError(capi.E_INVALID, "run_yuv_planes: uint8 device tensors [n, rows, cols]")
            return t
        y, u, v = plane(y), plane(u), plane(v)
        if not (y.shape[0] == u.shape[0] == v.shape[0]):
            raise HipError(capi.E_INVALID, "run_yuv_planes: the planes hold different numbers of frames")
        base = y.data_ptr()
        mk = lambda t: capi.YuvPlane(t.data_ptr() - base, t.stride(0) if t.shape[0] > 1 else 0, t.stride(1), t.stride(2))
        return base, y.shape[0], capi.YuvDesc(mk(y), mk(u), mk(v), sub_x, sub_y)

    def run_yuv_planes(self, y, u, v, sub_x=1, sub_y=1, scale=None, orient=0):
        """Three separately allocated planes (a software decoder's frame): y [n, H, W], u and v [n, ceil(H / 2^sub_y), ceil(W / 2^sub_x)].
        scale: the planes are the unreduced frame (run_yuv_resized; the plan is for resize_dims of y's size).  orient: the planes as
        stored (the plan is for oriented_dims of y's size); with both, turned upright and then reduced (oriented_resized_dims)."""
        base, n, desc = self.yuv_planes_desc(y, u, v, sub_x, sub_y)
        own = scale is not None or orient
        self._yuv_call(True, base, n, desc, y.shape[-2] if own else None, y.shape[-1] if own else None, orient, scale)

    def yuv_to_rgb8(self, base, n, rows, cols, desc):
        """The conversion alone on the device -> torch uint8 CUDA tensor [n][rows][cols][3] (acf_hip_yuv_to_rgb8; no model or plan)."""
        import torch
        out = torch.empty((n, rows, cols, 3), dtype=torch.uint8, device="cuda")
        self._chk(self.lib.acf_hip_yuv_to_rgb8(self.ctx, C.c_void_p(base if isinstance(base, int) else base.data_ptr()), n, rows, cols, C.byref(desc),
                                               C.c_void_p(out.data_ptr())))
        self.synchronize()
        return out

    def stream_open_yuv(self, desc, frame_bytes, cap=1024, depth=2, orient=0, src_rows=None, src_cols=None):
        """The streaming front end for host frames of frame_bytes each, described by desc (stride_n == frame_bytes).
        orient: frames as stored, src_rows x src_cols; every submit runs run_yuv(..., orient) on its slot."""
        self._yuv_open(desc, frame_bytes, cap, depth, src_rows, src_cols, orient)

    def stream_open_yuv_resized(self, desc, frame_bytes, src_rows, src_cols, scale, cap=1024, depth=2, orient=0):
        """stream_open_yuv for unreduced frames of src_rows x src_cols: every submit runs run_yuv_resized(..., orient) on its slot."""
        self._yuv_open(desc, frame_bytes, cap, depth, src_rows, src_cols, orient, scale)

    def _yuv_open(self, desc, frame_bytes, cap, depth, src_rows=None, src_cols=None, orient=0, scale=None):
        suffix, args = self._entry_for(src_rows, src_cols, orient, scale)
        self._chk(getattr(self.lib, "acf_hip_stream_open_yuv" + suffix)(self.ctx, C.byref(desc), frame_bytes, *args, cap, depth))
        self._stream_cap = cap

    # ---- video formats (acf_hip_yuv_format): 9 .. 16-bit samples, BT.709 / BT.2020, full range, beside the same descriptors
    @staticmethod
    def video_format(bits=8, shift=0, matrix="bt601", full_range=False):
        """capi.YuvFormat: bits 8 (bytes) or 9 .. 16 (little-endian words, sample = (word >> shift) & mask; P010: bits 10, shift 6),
        matrix "bt601" / "bt709" / "bt2020" or capi.YUV_MATRIX_*, full_range False = limited ("video")."""
        code = capi.YUV_MATRIX_NAMES.get(matrix.lower(), -1) if isinstance(matrix, str) else int(matrix)
        return capi.YuvFormat(int(bits), int(shift), code, int(full_range))

    @staticmethod
    def video_desc(layout, H, W, fmt=None, row_stride=0):
        """(capi.YuvDesc, frame bytes) of a named layout with the format's 1 or 2 bytes a sample (row_stride in bytes; 0 = tight)."""
        code = capi.YUV_NAMES.get(layout.lower(), -1) if isinstance(layout, str) else layout
        desc, fb = capi.YuvDesc(), C.c_int64()
        rc = capi.load().acf_hip_video_layout(code, C.byref(fmt) if fmt is not None else None, H, W, row_stride, C.byref(desc), C.byref(fb))
        if rc:
            raise HipError(rc, "acf_hip_video_layout(%r, %d x %d, stride %d)" % (layout, H, W, row_stride))
        return desc, fb.value

    @staticmethod
    def video_extent(desc, fmt, h, w, n):
        """([first Y, U, V], [last Y, U, V]): the lowest and highest BYTE offset from the base a call reads of each plane."""
        lo, hi = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        rc = capi.load().acf_hip_video_extent(C.byref(desc), C.byref(fmt) if fmt is not None else None, h, w, n, lo, hi)
        if rc:
            raise HipError(rc, "acf_hip_video_extent")
        return list(lo), list(hi)

    @staticmethod
    def yuv_coeffs(fmt=None):
        """[yoff, cmid, out_max, CY, CVR, CVG, CUG, CUB] of a format (host arithmetic)."""
        out = (C.c_int64 * 8)()
        rc = capi.load().acf_hip_yuv_coeffs(C.byref(fmt) if fmt is not None else None, out)
        if rc:
            raise HipError(rc, "acf_hip_yuv_coeffs")
        return list(out)

    def _video_args(self, fmt, src_rows, src_cols, orient, scale):
        """(format pointer, src_rows, src_cols, orient, scale) as the C entries take them: scale None = 0 = no resize; a size left
        out is the plan's, turned back, when the frame is turned, and 0 x 0 (the plain entry) otherwise."""
        if src_rows is None or src_cols is None:
            src_rows, src_cols = self._src_size(orient, None, None) if orient else (0, 0)
        return (C.byref(fmt) if fmt is not None else None), src_rows, src_cols, orient, float(scale) if scale is not None else 0.0

    def pyramid_video(self, base, n, desc, fmt=None, src_rows=None, src_cols=None, orient=0, scale=None):
        """pyramid_yuv / _oriented / _resized for frames of any capi.YuvFormat (fmt None: the default, the arithmetic of those entries).
        base: a torch device tensor (its first byte is the base) or a device pointer.  More than 8 bits: orient 0 and no scale."""
        ptr = C.c_void_p(base if isinstance(base, int) else base.data_ptr())
        self._chk(self.lib.acf_hip_pyramid_video(self.ctx, ptr, n, C.byref(desc), *self._video_args(fmt, src_rows, src_cols, orient, scale)))

    def run_video(self, base, n, desc, fmt=None, src_rows=None, src_cols=None, orient=0, scale=None):
        ptr = C.c_void_p(base if isinstance(base, int) else base.data_ptr())
        self._chk(self.lib.acf_hip_run_video(self.ctx, ptr, n, C.byref(desc), *self._video_args(fmt, src_rows, src_cols, orient, scale)))

    def video_to_rgb(self, base, n, rows, cols, desc, fmt=None):
        """The conversion alone on the device -> torch CUDA tensor [n][rows][cols][3] of R, G, B in [0, out_max]: uint8 for 8 bits,
        else 16-bit words (int16 storage: view them as uint16 on the host) (acf_hip_video_to_rgb; no model or plan)."""
        import torch
        wide = fmt is not None and fmt.bits > 8
        out = torch.empty((n, rows, cols, 3), dtype=torch.int16 if wide else torch.uint8, device="cuda")
        self._chk(self.lib.acf_hip_video_to_rgb(self.ctx, C.c_void_p(base if isinstance(base, int) else base.data_ptr()), n, rows, cols, C.byref(desc),
                                                C.byref(fmt) if fmt is not None else None, C.c_void_p(out.data_ptr())))
        self.synchronize()
        return out

    def stream_open_video(self, desc, fmt, frame_bytes, cap=1024, depth=2, src_rows=None, src_cols=None, orient=0, scale=None):
        """The streaming front end for host frames of frame_bytes each in any format: every submit runs run_video on its slot."""
        f, sr, sc, o, s = self._video_args(fmt, src_rows, src_cols, orient, scale)
        self._chk(self.lib.acf_hip_stream_open_video(self.ctx, C.byref(desc), f, frame_bytes, sr, sc, o, s, cap, depth))
        self._stream_cap = cap

    @staticmethod
    def video_planes_desc(y, u, v, sub_x, sub_y):
        """yuv_planes_desc for uint8 or 16-bit (int16 / uint16) torch device tensors [n, rows, cols]: strides in bytes."""
        def plane(t):
            if t.dim() == 2:
                t = t[None]
            if t.dim() != 3 or not t.is_cuda or t.element_size() != y.element_size() or t.element_size() > 2 or t.is_floating_point():
                raise HipError(capi.E_INVALID, "run_video_planes: uint8 or 16-bit integer device tensors [n, rows, cols] of one type")
            return t
        y, u, v = plane(y), plane(u), plane(v)
        if not (y.shape[0] == u.shape[0] == v.shape[0]):
            raise HipError(capi.E_INVALID, "run_video_planes: the planes hold different numbers of frames")
        base, es = y.data_ptr(), y.element_size()
        mk = lambda t: capi.YuvPlane(t.data_ptr() - base, es * t.stride(0) if t.shape[0] > 1 else 0, es * t.stride(1), es * t.stride(2))
        return base, y.shape[0], capi.YuvDesc(mk(y), mk(u), mk(v), sub_x, sub_y)

    def run_video_planes(self, y, u, v, sub_x=1, sub_y=1, fmt=None, scale=None, orient=0):
        """run_yuv_planes for any format: uint8 planes, or 16-bit planes with fmt.bits > 8 (upright and unreduced only)."""
        base, n, desc = self.video_planes_desc(y, u, v, sub_x, sub_y)
        own = scale is not None or orient
        self.run_video(base, n, desc, fmt, y.shape[-2] if own else None, y.shape[-1] if own else None, orient, scale)

    # ---- the apps' resize to a minimum object width (acf.cpp:117-148 Resizer) in front of the 8-bit entries
    @staticmethod
    def resize_scale(win_width, min_width):
        """scale = float(winSize.width) / float(minWidth), a float (acf.cpp:124)."""
        return float(np.float32(win_width) / np.float32(min_width))

    @staticmethod
    def resize_dims(rows, cols, scale):
        r, c_ = C.c_int(), C.c_int()
        rc = capi.load().acf_hip_resize_dims(rows, cols, float(scale), C.byref(r), C.byref(c_))
        if rc:
            raise HipError(rc, "acf_hip_resize_dims")
        return r.value, c_.value

    def set_input_resize(self, src_rows, src_cols, scale):
        """The plan must be for resize_dims(src_rows, src_cols, scale); the 8-bit entries then take src_rows x src_cols frames."""
        self._chk(self.lib.acf_hip_set_input_resize(self.ctx, src_rows, src_cols, float(scale)))

    def op_resize_u8(self, img, scale):
        """img: uint8 [rows][cols][cpp] (host) -> the reduced image (cv::resize as the apps' Resizer calls it)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        rows, cols, cpp = img.shape
        dr, dc = self.resize_dims(rows, cols, scale)
        out = np.zeros((dr, dc, cpp), dtype=np.uint8)
        self._chk(self.lib.acf_hip_op_resize_u8(self.ctx, img.ctypes.data, rows, cols, cpp, 0, float(scale), out.ctypes.data, dr, dc))
        return out

    @staticmethod
    def unscale_boxes(dets, scale):
        """Resizer::operator()(objects): cv::Rect2f(o) * (1.f / scale) -> cv::Rect (float products, cvRound); dets: DET_DTYPE array."""
        out = dets.copy()
        inv = np.float32(1.0) / np.float32(scale)
        for k in ("x", "y", "w", "h"):
            out[k] = np.rint((dets[k].astype(np.float32) * inv).astype(np.float64)).astype(out[k].dtype)
        return out

    # ---- rotated and mirrored frames (the oriented entries): host arithmetic
    @staticmethod
    def oriented_dims(src_rows, src_cols, orient):
        """(h, w) of the upright frame of a stored src_rows x src_cols frame: what the plan must be for."""
        h, w = C.c_int(), C.c_int()
        rc = capi.load().acf_hip_oriented_dims(src_rows, src_cols, orient, C.byref(h), C.byref(w))
        if rc:
            raise HipError(rc, "acf_hip_oriented_dims")
        return h.value, w.value

    @staticmethod
    def oriented_resized_dims(src_rows, src_cols, orient, scale):
        """(h, w) of the reduced upright frame of a stored src_rows x src_cols frame: resize_dims(oriented_dims(...), scale)."""
        h, w = C.c_int(), C.c_int()
        rc = capi.load().acf_hip_oriented_resized_dims(src_rows, src_cols, orient, float(scale), C.byref(h), C.byref(w))
        if rc:
            raise HipError(rc, "acf_hip_oriented_resized_dims")
        return h.value, w.value

    @staticmethod
    def unorient_boxes(dets, orient, src_rows, src_cols):
        """Boxes of the upright frame -> the boxes covering the same pixels in the stored frame (acf_hip_unorient_rect); dets: DET_DTYPE array."""
        out = dets.copy()
        lib = capi.load()
        a, b = (C.c_int32 * 4)(), (C.c_int32 * 4)()
        for i in range(len(dets)):
            a[:] = [int(dets[k][i]) for k in ("x", "y", "w", "h")]
            rc = lib.acf_hip_unorient_rect(orient, src_rows, src_cols, a, b)
            if rc:
                raise HipError(rc, "acf_hip_unorient_rect")
            for j, k in enumerate(("x", "y", "w", "h")):
                out[k][i] = b[j]
        return out

    # ---- crops of the stored frame under boxes or the last batch's detections (acf_hip_cut_crops / acf_hip_cut_detections)
    @staticmethod
    def _crop_source(ptr, n, image, yuv, fmt, src_rows, src_cols, orient, keep):
        src = capi.CropSource(C.c_void_p(ptr), n, C.pointer(image) if image is not None else None, C.pointer(yuv) if yuv is not None else None,
                              C.pointer(fmt) if fmt is not None else None, src_rows, src_cols, orient)
        src.keep = (image, yuv, fmt, keep)    # what the pointers point at lives as long as the source
        src.channels = int(image.channels) if image is not None else 3
        bits = int(fmt.bits) if fmt is not None else 8
        src.sample_bytes = {capi.T_F16: 2, capi.T_BF16: 2, capi.T_F32: 4}.get(int(image.dtype), 1) if image is not None else (1 if bits == 8 else 2)
        src.floating = image is not None and int(image.dtype) != capi.T_U8
        return src

    def crop_source_tensor(self, t, layout="nchw", orient=0):
        """capi.CropSource of a device tensor [n, c, Hs, Ws] ("nhwc": [n, Hs, Ws, c]) of any strides holding the frames AS STORED,
        uint8 / float16 / bfloat16 / float32; orient: capi.ORIENT_*.  Nothing is copied."""
        if layout not in ("nchw", "nhwc") or t.dim() != 4 or not t.is_cuda:
            raise HipError(capi.E_INVALID, "crop_source_tensor: a device tensor of four dimensions, layout \"nchw\" or \"nhwc\"")
        if layout == "nhwc":
            t = t.permute(0, 3, 1, 2)
        n, ch, h, w = t.shape
        sn, sc, sy, sx = t.stride()
        return self._crop_source(t.data_ptr(), n, capi.ImageDesc(self._torch_dtype_code(t), ch, sn, sc, sy, sx), None, None, h, w, orient, t)

    def crop_source_image(self, ptr, n, desc, src_rows, src_cols, orient=0):
        """capi.CropSource of a raw device pointer and a capi.ImageDesc (what no torch view expresses: a negative channel stride)."""
        return self._crop_source(ptr, n, desc, None, None, src_rows, src_cols, orient, None)

    def crop_source_yuv(self, base, n, desc, fmt=None, src_rows=None, src_cols=None, orient=0):
        """capi.CropSource of video frames as run_video reads them: base a torch device tensor (its first byte is the base) or a
        device pointer, desc a capi.YuvDesc at src_rows x src_cols (the stored size), fmt a capi.YuvFormat or None (the default)."""
        ptr = base if isinstance(base, int) else base.data_ptr()
        return self._crop_source(ptr, n, None, desc, fmt, src_rows, src_cols, orient, base)

    @staticmethod
    def crop_spec(out_size, samples=1, dtype=None, layout="planar", k=1, grow=1.0):
        """capi.CropSpec: out_size (h, w) or one number; dtype a torch dtype, capi.T_* or None (float32); layout "planar" [C][h][w] or
        "packed" [h][w][C]."""
        oh, ow = (out_size, out_size) if isinstance(out_size, int) else out_size
        if dtype is None:
            dtype = capi.T_F32
        elif not isinstance(dtype, int):
            import torch
            dtype = {torch.uint8: capi.T_U8, torch.float16: capi.T_F16, torch.bfloat16: capi.T_BF16, torch.float32: capi.T_F32}.get(dtype, -1)
        lay = {"planar": 0, "packed": 1}.get(layout, -1) if isinstance(layout, str) else int(layout)
        return capi.CropSpec(int(oh), int(ow), int(samples), dtype, lay, int(k), float(grow), 0)

    @staticmethod
    def _crop_tensor(spec, channels, lead):
        import torch
        dt = {capi.T_U8: torch.uint8, capi.T_F16: torch.float16, capi.T_BF16: torch.bfloat16, capi.T_F32: torch.float32}.get(int(spec.dtype), torch.float32)
        shape = (spec.out_h, spec.out_w, channels) if spec.layout == 1 else (channels, spec.out_h, spec.out_w)
        return torch.empty(tuple(lead) + tuple(max(int(v), 0) for v in shape), dtype=dt, device="cuda")

    def cut_crops(self, source, boxes, frame_index, out_size, samples=1, dtype=None, layout="planar", out=None):
        """Crop i of box boxes[i] = (x, y, w, h) in the upright frame of stored frame frame_index[i] of `source` -> torch device tensor
        [n, C, oh, ow] (layout "packed": [n, oh, ow, C]).  boxes float32 [n, 4], frame_index int32 [n]: device tensors (host arrays
        are copied over first).  Asynchronous on the context's stream; no model or plan.  out: a tensor to write into."""
        import torch
        spec = self.crop_spec(out_size, samples, dtype, layout)
        if not torch.is_tensor(boxes):
            boxes = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).cuda()
        if not torch.is_tensor(frame_index):
            frame_index = torch.from_numpy(np.ascontiguousarray(frame_index, dtype=np.int32)).cuda()
        n = int(frame_index.shape[0])
        if boxes.dtype != torch.float32 or frame_index.dtype != torch.int32 or tuple(boxes.shape) != (n, 4) or not boxes.is_contiguous() \
                or not frame_index.is_contiguous() or not boxes.is_cuda or not frame_index.is_cuda:
            raise HipError(capi.E_INVALID, "cut_crops: boxes float32 [n, 4] and frame_index int32 [n], contiguous device tensors")
        if out is None:
            out = self._crop_tensor(spec, source.channels, (n,))
        self._chk(self.lib.acf_hip_cut_crops(self.ctx, C.byref(source), C.c_void_p(boxes.data_ptr()), C.c_void_p(frame_index.data_ptr()), n, C.byref(spec),
                                             C.c_void_p(out.data_ptr())))
        return out

    def cut_detections(self, source, out_size, k, det_scale=None, grow=1.0, samples=1, dtype=None, layout="planar", out=None, boxes_out=None,
                       counts_out=None):
        """The first k detections of every frame of the last detect / run* call, cropped out of `source` (the frames that call read,
        as stored) -> (crops [nF, k, C, oh, ow] (or [nF, k, oh, ow, C]), boxes float32 [nF, k, 4] in the upright frame, counts int32
        [nF]), all on the device, nothing synchronised; slots at and beyond a frame's count are not written.  det_scale: the scale
        the frames were reduced by (None: none); grow: the box grown about its centre."""
        import torch
        spec = self.crop_spec(out_size, samples, dtype, layout, k, grow)
        nF = int(source.n_frames)
        if out is None:
            out = self._crop_tensor(spec, source.channels, (nF, max(int(k), 0)))
        if boxes_out is None:
            boxes_out = torch.empty((nF, max(int(k), 0), 4), dtype=torch.float32, device="cuda")
        if counts_out is None:
            counts_out = torch.empty((nF,), dtype=torch.int32, device="cuda")
        self._chk(self.lib.acf_hip_cut_detections(self.ctx, C.byref(source), float(det_scale) if det_scale is not None else 0.0, C.byref(spec),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(boxes_out.data_ptr()), C.c_void_p(counts_out.data_ptr())))
        return out, boxes_out, counts_out

    @staticmethod
    def crop_box(det, det_scale=None, grow=1.0):
        """A detection (x, y, w, h) of the reduced frame -> float32 [4], its box in the upright frame grown about its centre
        (acf_hip_crop_box: cv::Rect2f(o) * (1.f / scale), as the apps map boxes back)."""
        a = (C.c_int32 * 4)(*[int(v) for v in det])
        out = np.zeros(4, dtype=np.float32)
        rc = capi.load().acf_hip_crop_box(a, float(det_scale) if det_scale is not None else 0.0, float(grow), capi.fptr(out))
        if rc:
            raise HipError(rc, "acf_hip_crop_box")
        return out

    @staticmethod
    def crop_bytes(spec, channels):
        out = C.c_int64()
        rc = capi.load().acf_hip_crop_bytes(C.byref(spec), channels, C.byref(out))
        if rc:
            raise HipError(rc, "acf_hip_crop_bytes")
        return out.value

    @staticmethod
    def crop_form(spec, box, Hu, Wu, channels, sample_bytes):
        """0 staged, 1 gather: the form k_cut_crops takes for this box (host arithmetic)."""
        b = np.ascontiguousarray(box, dtype=np.float32)
        out = C.c_int()
        rc = capi.load().acf_hip_crop_form(C.byref(spec), capi.fptr(b), Hu, Wu, channels, sample_bytes, C.byref(out))
        if rc:
            raise HipError(rc, "acf_hip_crop_form")
        return out.value

    # ---- affine views of the stored frame as the batch's frames (acf_hip_pyramid_view / acf_hip_run_view)
    def _view_call(self, detect, source, views, frames, samples):
        import torch
        if not torch.is_tensor(views):
            views = torch.from_numpy(np.ascontiguousarray(views, dtype=np.float32).reshape(-1, 6)).cuda()
        if frames is not None and not torch.is_tensor(frames):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.int32)).cuda()
        n = int(views.shape[0])
        if views.dtype != torch.float32 or views.dim() != 2 or views.shape[1] != 6 or not views.is_contiguous() or not views.is_cuda:
            raise HipError(capi.E_INVALID, "run_view: views float32 [n, 6], a contiguous device tensor")
        if frames is not None and (frames.dtype != torch.int32 or tuple(frames.shape) != (n,) or not frames.is_contiguous() or not frames.is_cuda):
            raise HipError(capi.E_INVALID, "run_view: frames int32 [n], a contiguous device tensor")
        fn = self.lib.acf_hip_run_view if detect else self.lib.acf_hip_pyramid_view
        self._chk(fn(self.ctx, C.byref(source), C.c_void_p(views.data_ptr()), C.c_void_p(frames.data_ptr()) if frames is not None else None, n, int(samples)))
        self._view_keep = (views, frames)     # the call is asynchronous: what it reads lives until the next one

    def pyramid_view(self, source, views, frames=None, samples=1):
        """The pyramid of views of stored frames: frame i of the batch is the affine view views[i] (six floats: xu = m0 x + m1 y + m2,
        yu = m3 x + m4 y + m5 from the plan's frame into the upright stored frame) of stored frame frames[i] (None: frame i) of
        `source` (crop_source_tensor / crop_source_yuv), samples x samples bilinear samples a pixel.  views, frames: numpy arrays
        (copied over first) or device tensors."""
        self._view_call(False, source, views, frames, samples)

    def run_view(self, source, views, frames=None, samples=1):
        """pyramid_view, then the cascade.  The detections are in VIEW coordinates: view_quad / view_box map them back on the host,
        merge_views maps and merges them into their stored frames on the device (and feeds cut_crops from there)."""
        self._view_call(True, source, views, frames, samples)

    # ---- the views' detections merged into their stored frames (acf_hip_merge_views / acf_hip_op_merge_views)
    @staticmethod
    def merge_spec(nms=None, k=64, grow=1.0):
        """capi.MergeSpec: nms a capi.NmsParams (capi.make_nms) applied across the views of one stored frame, or None (type 0: every
        mapped detection in view order); k records per stored frame; grow: boxes_out grown about their centres."""
        spec = capi.MergeSpec()
        spec.nms = nms if nms is not None else capi.make_nms("none")
        spec.max_per_frame, spec.grow = int(k), float(grow)
        return spec

    def merge_views(self, views, frames=None, n_frames=None, nms=None, k=64, grow=1.0, quads=False):
        """The detections of the last run_view mapped into the upright stored frames and merged across the views of each stored frame
        (bbNms's rule on the mapped boxes), on the device: views, frames as run_view was given them (numpy arrays are copied over
        first), n_frames the stored frames (None: the number of views).  -> (records: uint8 [n_frames, k, 32] holding
        capi.MERGED_DTYPE, counts int32 [n_frames] (the true number of survivors; -1: a frame over capacity), boxes float32
        [n_frames, k, 4] grown by `grow`, frame_index int32 [n_frames, k], and with quads=True quads float32 [n_frames, k, 4, 2]), all
        device tensors, nothing synchronised.  Record and quad slots at and beyond min(count, k) are NOT written: their content is
        undefined.  boxes and frame_index are written in EVERY slot (zeros and -1 beyond the count):
        cut_crops(source, boxes.view(-1, 4), frame_index.view(-1), ...) is the device-only route to crops."""
        import torch
        if not torch.is_tensor(views):
            views = torch.from_numpy(np.ascontiguousarray(views, dtype=np.float32).reshape(-1, 6)).cuda()
        if frames is not None and not torch.is_tensor(frames):
            frames = torch.from_numpy(np.ascontiguousarray(frames, dtype=np.int32)).cuda()
        n = int(views.shape[0])
        if views.dtype != torch.float32 or views.dim() != 2 or views.shape[1] != 6 or not views.is_contiguous() or not views.is_cuda:
            raise HipError(capi.E_INVALID, "merge_views: views float32 [n, 6], a contiguous device tensor")
        if frames is not None and (frames.dtype != torch.int32 or tuple(frames.shape) != (n,) or not frames.is_contiguous() or not frames.is_cuda):
            raise HipError(capi.E_INVALID, "merge_views: frames int32 [n], a contiguous device tensor")
        nF = n if n_frames is None else int(n_frames)
        spec = self.merge_spec(nms, k, grow)
        kk, ff = max(int(k), 0), max(nF, 0)
        # (torch.empty, never a fill: a fill would run on torch's stream, unordered with the kernel on the context's)
        rec = torch.empty((ff, kk, capi.MERGED_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        counts = torch.empty((ff,), dtype=torch.int32, device="cuda")
        boxes = torch.empty((ff, kk, 4), dtype=torch.float32, device="cuda")
        fidx = torch.empty((ff, kk), dtype=torch.int32, device="cuda")
        qd = torch.empty((ff, kk, 4, 2), dtype=torch.float32, device="cuda") if quads else None
        self._chk(self.lib.acf_hip_merge_views(self.ctx, C.c_void_p(views.data_ptr()), C.c_void_p(frames.data_ptr()) if frames is not None else None, n, nF,
                                               C.byref(spec), C.c_void_p(rec.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(boxes.data_ptr()),
                                               C.c_void_p(fidx.data_ptr()), C.c_void_p(qd.data_ptr()) if quads else None))
        self._merge_keep = (views, frames)    # the call is asynchronous: what it reads lives until the next one
        return (rec, counts, boxes, fidx, qd) if quads else (rec, counts, boxes, fidx)

    def op_merge_views(self, dets, counts, views, frames=None, n_frames=None, nms=None, k=64, grow=1.0, fill=None):
        """The same kernel on host lists: dets capi.DET_DTYPE [n_views, max_hits], counts int32 [n_views], views float32 [n_views, 6],
        frames int32 [n_views] or None -> numpy (records capi.MERGED_DTYPE [n_frames, k], counts int32 [n_frames], boxes float32
        [n_frames, k, 4], frame_index int32 [n_frames, k], quads float32 [n_frames, k, 4, 2]).  fill: a byte the outputs hold before
        the call (None: 0) — slots the kernel does not write keep it."""
        dets = np.ascontiguousarray(dets, dtype=capi.DET_DTYPE)
        views = np.ascontiguousarray(views, dtype=np.float32).reshape(-1, 6)
        n = len(views)
        dets = dets.reshape(n, -1)
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(n)
        fr = None if frames is None else np.ascontiguousarray(frames, dtype=np.int32).reshape(n)
        nF = n if n_frames is None else int(n_frames)
        spec = self.merge_spec(nms, k, grow)
        kk, ff, b = max(int(k), 0), max(nF, 0), 0 if fill is None else int(fill)
        rec = np.full((ff, kk, capi.MERGED_DTYPE.itemsize), b, dtype=np.uint8)
        cnt = np.full((ff, 4), b, dtype=np.uint8)
        boxes = np.full((ff, kk, 16), b, dtype=np.uint8)
        fidx = np.full((ff, kk, 4), b, dtype=np.uint8)
        qd = np.full((ff, kk, 32), b, dtype=np.uint8)
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        self._chk(self.lib.acf_hip_op_merge_views(self.ctx, ptr(dets), ptr(counts), dets.shape[1], ptr(views), ptr(fr), n, nF, C.byref(spec), ptr(rec), ptr(cnt),
                                                  ptr(boxes), ptr(fidx), ptr(qd)))
        return (rec.view(capi.MERGED_DTYPE).reshape(ff, kk), cnt.view(np.int32).reshape(ff), boxes.view(np.float32).reshape(ff, kk, 4),
                fidx.view(np.int32).reshape(ff, kk), qd.view(np.float32).reshape(ff, kk, 4, 2))

    # ---- a bank of classifiers on one pyramid (acf_hip_set_bank / _detect_bank / _join_bank)
    @staticmethod
    def bank_check(primary, member):
        """acf_hip_bank_check on two model dicts -> (code, reason): capi.OK, or why `member` cannot share `primary`'s pyramid."""
        pp, keep_p = capi.make_params(primary)
        pm, keep_m = capi.make_params(member)
        why = C.create_string_buffer(512)
        rc = capi.load().acf_hip_bank_check(C.byref(pp), C.byref(pm), why, len(why))
        del keep_p, keep_m
        return rc, why.value.decode()

    def set_bank(self, models):
        """The bank's members (model dicts sharing every pyramid and channel field with the context's model; at most capi.BANK_MAX; an
        empty list clears the bank).  Drops the plan: call plan() again."""
        made = [capi.make_params(m) for m in models]
        arr = (capi.Params * max(len(made), 1))(*[p for p, _ in made])
        self._chk(self.lib.acf_hip_set_bank(self.ctx, arr if made else None, len(made)))
        self.bank_models = list(models)
        self.levels = []

    def detect_bank(self):
        """Every member's cascade on the pyramid of the last batch (after any pyramid* / run* entry), asynchronously."""
        self._chk(self.lib.acf_hip_detect_bank(self.ctx))

    def bank_detections(self, model, frame):
        """Model `model`'s raw list of one frame after detect_bank (model 0: raw_detections)."""
        det = np.zeros(self.max_hits, dtype=capi.DET_DTYPE)
        n = C.c_int()
        self._chk(self.lib.acf_hip_get_bank_detections(self.ctx, model, frame, det.ctypes.data_as(C.POINTER(capi.Detection)), self.max_hits, C.byref(n)))
        return det[:n.value].copy()

    def bank_hits(self, model, frame):
        hits = np.zeros(self.max_hits, dtype=capi.HIT_DTYPE)
        n = C.c_int()
        self._chk(self.lib.acf_hip_get_bank_hits(self.ctx, model, frame, hits.ctypes.data_as(C.POINTER(capi.Hit)), self.max_hits, C.byref(n)))
        return hits[:n.value].copy()

    def bank_forms(self, model):
        """cascade_forms() of model `model`'s last cascade (None before its first)."""
        n = C.c_int()
        out = (C.c_int32 * capi.CF_WORDS)()
        self._chk(self.lib.acf_hip_get_bank_forms(self.ctx, model, out, capi.CF_WORDS, C.byref(n)))
        return self._cascade_forms_of([int(v) for v in out])

    def bank_levels(self, model):
        """The plan's levels with model `model`'s window grid."""
        lv = (capi.Level * len(self.levels))()
        self._chk(self.lib.acf_hip_get_bank_levels(self.ctx, model, lv, len(self.levels)))
        return list(lv)

    @staticmethod
    def bank_spec(nms=None, separate=False, k=64, grow=1.0, det_scale=None):
        """capi.BankSpec: nms a capi.NmsParams applied across the models of one frame (separate: within each model), or None (type 0:
        the lists concatenated); k records per frame; grow, det_scale: crop_box's, for boxes_out."""
        spec = capi.BankSpec()
        spec.nms = nms if nms is not None else capi.make_nms("none")
        spec.separate, spec.max_per_frame, spec.grow = int(separate), int(k), float(grow)
        spec.det_scale = 0.0 if det_scale is None else float(det_scale)
        return spec

    def join_bank(self, nms=None, separate=False, k=64, grow=1.0, det_scale=None):
        """The lists of the last run* + detect_bank joined per frame on the device -> (records: uint8 [n_frames, k, 32] holding
        capi.BANK_DTYPE, counts int32 [n_frames] (the true number of survivors; -1: an unknowable frame), boxes float32 [n_frames, k, 4]
        = crop_box(det, det_scale, grow), frame_index int32 [n_frames, k]), all device tensors, nothing synchronised.  Record slots at
        and beyond min(count, k) are NOT written; boxes and frame_index are written in EVERY slot (zeros and -1 beyond the count):
        cut_crops(source, boxes.view(-1, 4), frame_index.view(-1), ...) is the device-only route to crops."""
        import torch
        spec = self.bank_spec(nms, separate, k, grow, det_scale)
        # sized for the plan's batch: the kernel writes the frames of the context's last batch, never more than max_batch
        kk, ff = max(int(k), 0), int(self.max_batch)
        rec = torch.empty((ff, kk, capi.BANK_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        counts = torch.empty((ff,), dtype=torch.int32, device="cuda")
        boxes = torch.empty((ff, kk, 4), dtype=torch.float32, device="cuda")
        fidx = torch.empty((ff, kk), dtype=torch.int32, device="cuda")
        self._chk(self.lib.acf_hip_join_bank(self.ctx, C.byref(spec), C.c_void_p(rec.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(boxes.data_ptr()),
                                             C.c_void_p(fidx.data_ptr())))
        n = self._bank_frames()
        return rec[:n], counts[:n], boxes[:n], fidx[:n]

    def _bank_frames(self):
        """Frames of the last detect_bank, to slice join_bank's outputs (which are allocated for max_batch frames, so this number
        sizes nothing): the first member's cascade record holds them (a member runs nothing else)."""
        out = (C.c_int32 * capi.CF_WORDS)()
        n = C.c_int()
        rc = self.lib.acf_hip_get_bank_forms(self.ctx, 1, out, capi.CF_WORDS, C.byref(n))
        return min(int(out[29]), int(self.max_batch)) if rc == capi.OK and int(out[29]) > 0 else int(self.max_batch)

    def op_join_bank(self, dets, counts, nms=None, separate=False, k=64, grow=1.0, det_scale=None, fill=None):
        """The same kernel on host lists: dets capi.DET_DTYPE [n_models, n_frames, max_hits], counts int32 [n_models, n_frames] ->
        numpy (records capi.BANK_DTYPE [n_frames, k], counts int32 [n_frames], boxes float32 [n_frames, k, 4], frame_index int32
        [n_frames, k]).  fill: a byte the outputs hold before the call (None: 0) — slots the kernel does not write keep it."""
        dets = np.ascontiguousarray(dets, dtype=capi.DET_DTYPE)
        assert dets.ndim == 3
        nM, nF, mh = dets.shape
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(nM, nF)
        spec = self.bank_spec(nms, separate, k, grow, det_scale)
        kk, b = max(int(k), 0), 0 if fill is None else int(fill)
        rec = np.full((nF, kk, capi.BANK_DTYPE.itemsize), b, dtype=np.uint8)
        cnt = np.full((nF, 4), b, dtype=np.uint8)
        boxes = np.full((nF, kk, 16), b, dtype=np.uint8)
        fidx = np.full((nF, kk, 4), b, dtype=np.uint8)
        ptr = lambda a: C.c_void_p(a.ctypes.data)
        self._chk(self.lib.acf_hip_op_join_bank(self.ctx, ptr(dets), ptr(counts), nM, nF, mh, C.byref(spec), ptr(rec), ptr(cnt), ptr(boxes), ptr(fidx)))
        return (rec.view(capi.BANK_DTYPE).reshape(nF, kk), cnt.view(np.int32).reshape(nF), boxes.view(np.float32).reshape(nF, kk, 4),
                fidx.view(np.int32).reshape(nF, kk))

    @staticmethod
    def view_from_box(box, angle_rad, h, w):
        """float32 [6]: the view whose h x w frame is the box (x, y, w, h in the upright stored frame) turned by angle_rad about its centre."""
        b, m = np.ascontiguousarray(box, dtype=np.float32), np.zeros(6, dtype=np.float32)
        rc = capi.load().acf_hip_view_from_box(capi.fptr(b), float(angle_rad), int(h), int(w), capi.fptr(m))
        if rc:
            raise HipError(rc, "acf_hip_view_from_box")
        return m

    @staticmethod
    def view_quad(m, det):
        """A detection (x, y, w, h) of the view's frame -> float32 [4, 2]: its corners TL, TR, BR, BL (x, y) in the upright stored frame."""
        mm, q = np.ascontiguousarray(m, dtype=np.float32), np.zeros(8, dtype=np.float32)
        rc = capi.load().acf_hip_view_quad(capi.fptr(mm), (C.c_int32 * 4)(*[int(v) for v in det]), capi.fptr(q))
        if rc:
            raise HipError(rc, "acf_hip_view_quad")
        return q.reshape(4, 2)

    @staticmethod
    def view_box(m, det):
        """A detection of the view's frame -> float32 [4]: the bounding box (x, y, w, h) of view_quad, what cut_crops takes."""
        mm, b = np.ascontiguousarray(m, dtype=np.float32), np.zeros(4, dtype=np.float32)
        rc = capi.load().acf_hip_view_box(capi.fptr(mm), (C.c_int32 * 4)(*[int(v) for v in det]), capi.fptr(b))
        if rc:
            raise HipError(rc, "acf_hip_view_box")
        return b

    @staticmethod
    def view_form(m, samples, tile_x, tile_y, h, w, Hu, Wu, channels, sample_bytes):
        """0 staged, 1 gather: the form k_ingest_view takes for a 64 x 64 tile of the h x w frame (host arithmetic)."""
        mm, out = np.ascontiguousarray(m, dtype=np.float32), C.c_int()
        rc = capi.load().acf_hip_view_form(capi.fptr(mm), samples, tile_x, tile_y, h, w, Hu, Wu, channels, sample_bytes, C.byref(out))
        if rc:
            raise HipError(rc, "acf_hip_view_form")
        return out.value

    # ---- streaming front end (pinned host frames in, pinned host records out)
    def stream_open(self, pix=capi.PIX_RGB, row_stride=0, cap=1024, depth=2):
        self._chk(self.lib.acf_hip_stream_open(self.ctx, pix, row_stride, cap, depth))
        self._stream_cap = cap

    def stream_submit(self, host_ptr, n):
        t = C.c_int()
        self._chk(self.lib.acf_hip_stream_submit(self.ctx, C.c_void_p(host_ptr), n, C.byref(t)))
        return t.value

    def stream_collect(self, ticket):
        """-> int32 array [n][1 + 6*cap] (a copy of the pinned records: count, then {x,y,w,h,score bits,scale})."""
        rec = C.POINTER(C.c_int32)()
        n = C.c_int()
        self._chk(self.lib.acf_hip_stream_collect(self.ctx, ticket, C.byref(rec), C.byref(n)))
        per = 1 + 6 * self._stream_cap
        return np.ctypeslib.as_array(rec, shape=(n.value, per)).copy()

    def stream_close(self):
        self._chk(self.lib.acf_hip_stream_close(self.ctx))

    def synchronize(self):
        self._chk(self.lib.acf_hip_synchronize(self.ctx))

    def repairs(self):
        """(smoothing planes checked, recomputed, level planes checked, recomputed) with option count_repairs on."""
        out = (C.c_int64 * 4)()
        self._chk(self.lib.acf_hip_get_repairs(self.ctx, out))
        return tuple(int(x) for x in out)

    def tri_forms(self):
        """Per real scale, the form convTri(M, normRad) took in the last call (acf_hip_get_tri_forms): bit 0 = checkpoints replayed by the
        y kernel, bit 1 = a plane U is held."""
        cap = 64
        n = C.c_int()
        out = (C.c_int32 * cap)()
        self._chk(self.lib.acf_hip_get_tri_forms(self.ctx, out, cap, C.byref(n)))
        return [int(out[i]) for i in range(min(n.value, cap))]

    LEVEL_PATHS = ("fused", "wave_smooth", "smooth_jobs", "copy")
    LEVEL_MODES = ("real", "dd", "du", "ud", "uu")
    LEVEL_TAKERS = (None, "all", "group")
    LEVEL_WHY = ("taps", "exact", "rows", "window", "tall", "mixed")

    def level_forms(self):
        """What the level stage decided (acf_hip_get_level_forms): dict(path, emit_rank, emit_f32, segments, approx_first, levels), of the
        last pyramid call (before the first: the call-wide entries are zero / "fused" / False and the levels are the plan's fused list); levels[i] = dict(R, mode, by = "all" (k_level_all) / "group" (a k_level<R, mode> launch) / None, why = the
        reasons level i gives the plan not to fuse, a tuple of LEVEL_WHY names)."""
        cap = capi.LF_HEAD + 256
        n = C.c_int()
        out = (C.c_int32 * cap)()
        self._chk(self.lib.acf_hip_get_level_forms(self.ctx, out, cap, C.byref(n)))
        levels = []
        for i in range(capi.LF_HEAD, min(n.value, cap)):
            w = int(out[i])
            levels.append(dict(R=w & 255, mode=self.LEVEL_MODES[w >> 8 & 7], by=self.LEVEL_TAKERS[w >> 12 & 3],
                               why=tuple(name for b, name in enumerate(self.LEVEL_WHY) if w >> (16 + b) & 1)))
        assert out[5] in (0, len(levels))   # (the call-wide words are zero before the first pyramid call)
        return dict(path=self.LEVEL_PATHS[out[0]], emit_rank=bool(out[1]), emit_f32=bool(out[2]), segments=int(out[3]),
                    approx_first=bool(out[4]), levels=levels)

    SCALE_ROUTES = ("none", "half_fused", "pair_b", "strip", "strip_pair_a", "half", "up", "generic")
    STRIP_WHY = (None, "not_down", "rows", "align", "pair_mismatch", "slow_taps", "x_taps", "b_steps", "no_tiling")

    def scale_forms(self):
        """How each real scale's image was resampled (acf_hip_get_scale_forms): per real scale dict(route = a SCALE_ROUTES name of the
        last pyramid call ("none" before the first), slow, xt2, nty, n_split of the launch it made, plan_strip / plan_pair = the plan
        holds a strip plan of the scale alone / with the next scale, why / why_pair = the STRIP_WHY name of the plan's refusal or None)."""
        cap = 64
        n = C.c_int()
        out = (C.c_int32 * cap)()
        self._chk(self.lib.acf_hip_get_scale_forms(self.ctx, out, cap, C.byref(n)))
        forms = []
        for i in range(min(n.value, cap)):
            w = int(out[i]) & 0xffffffff
            forms.append(dict(route=self.SCALE_ROUTES[w & 15], slow=bool(w >> 4 & 1), xt2=bool(w >> 5 & 1), plan_strip=bool(w >> 6 & 1),
                              plan_pair=bool(w >> 7 & 1), nty=w >> 8 & 255, n_split=w >> 16 & 255, why=self.STRIP_WHY[w >> 24 & 15],
                              why_pair=self.STRIP_WHY[w >> 28 & 15]))
        return forms

    CASCADE_PATHS = ("none", "tiled2", "staged")
    CASCADE_TILE_KERNELS = (None, "tile3", "tile3D", "tileD")

    def cascade_forms(self):
        """What the last cascade call decided (acf_hip_get_cascade_forms; the pipeline's or the operator's, whichever ran last; None
        before the first): dict(path = a CASCADE_PATHS name, rank, kernel = a CASCADE_TILE_KERNELS name, NW, TR, TC, passW, pooled, b,
        nTiles, blocks, persist, tileLds, nStages, bounds, firstStage, mode, codeScan, pooledTail, waveTail, codes_cap, qcap, frames)."""
        n = C.c_int()
        out = (C.c_int32 * capi.CF_WORDS)()
        self._chk(self.lib.acf_hip_get_cascade_forms(self.ctx, out, capi.CF_WORDS, C.byref(n)))
        assert n.value == capi.CF_WORDS
        return self._cascade_forms_of([int(v) for v in out])

    @classmethod
    def _cascade_forms_of(self, w):
        if w[29] == 0:
            return None
        return dict(path=self.CASCADE_PATHS[w[0]], rank=bool(w[1]), kernel=self.CASCADE_TILE_KERNELS[w[2]], NW=w[3], TR=w[4], TC=w[5], passW=w[6],
                    pooled=bool(w[7]), b=tuple(w[8:13]), nTiles=w[13], blocks=w[14], persist=bool(w[15]), tileLds=w[16], nStages=w[17],
                    bounds=tuple(w[18:22]), firstStage=w[22], mode=w[23], codeScan=bool(w[24]), pooledTail=bool(w[25]), waveTail=bool(w[26]),
                    codes_cap=w[27], qcap=w[28], frames=w[29])

    def set_option(self, key, value):
        self._chk(self.lib.acf_hip_set_option(self.ctx, key.encode(), int(value)))

    def set_x86_tables(self, rcp, rsqrt):
        """Install one x86 CPU's _mm_rcp_ps / _mm_rsqrt_ps tables (4096 + 2 x 4096 uint32, acf_hip_set_x86_tables); option "arith" = 1
        then makes the reference's three approximate sites return that CPU's bits."""
        rcp = np.ascontiguousarray(rcp, dtype=np.uint32)
        rsqrt = np.ascontiguousarray(rsqrt, dtype=np.uint32)
        assert rcp.shape == (4096,) and rsqrt.shape == (8192,)
        u32p = C.POINTER(C.c_uint32)
        self._chk(self.lib.acf_hip_set_x86_tables(self.ctx, rcp.ctypes.data_as(u32p), rsqrt.ctypes.data_as(u32p)))

    def selftest_x86(self, first, count, stride=1):
        """(rcp digest, rsqrt digest, mismatches of gradMag's one-read form) of the device's table functions over first + i * stride."""
        out = (C.c_uint64 * 3)()
        self._chk(self.lib.acf_hip_selftest_x86(self.ctx, C.c_uint32(first), C.c_uint64(count), C.c_uint32(stride), out))
        return int(out[0]), int(out[1]), int(out[2])

    def profile(self):
        """{kernel name: (total ms, launches)} since the last call (option "profile")."""
        cap = 64
        n = C.c_int()
        names = (C.c_char_p * cap)()
        ms = (C.c_float * cap)()
        cnt = (C.c_int * cap)()
        self._chk(self.lib.acf_hip_profile_get(self.ctx, C.byref(n), names, ms, cnt, cap))
        return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(min(n.value, cap))}

    def export_detections(self, dst, cap):
        self._chk(self.lib.acf_hip_export_detections(self.ctx, C.c_void_p(dst.data_ptr()), cap))

    def detections(self, frame):
        det = np.zeros(self.max_hits, dtype=capi.DET_DTYPE)
        hits = np.zeros(self.max_hits, dtype=capi.HIT_DTYPE)
        n = C.c_int()
        self._chk(self.lib.acf_hip_get_detections(self.ctx, frame, det.ctypes.data_as(C.POINTER(capi.Detection)), self.max_hits, C.byref(n)))
        self._chk(self.lib.acf_hip_get_hits(self.ctx, frame, hits.ctypes.data_as(C.POINTER(capi.Hit)), self.max_hits, C.byref(n)))
        return det[:n.value].copy(), hits[:n.value].copy()

    def raw_detections(self, frame):
        """acfDetect1's list (scale, column, row order) whether or not the device NMS is on."""
        det = np.zeros(self.max_hits, dtype=capi.DET_DTYPE)
        n = C.c_int()
        self._chk(self.lib.acf_hip_get_raw_detections(self.ctx, frame, det.ctypes.data_as(C.POINTER(capi.Detection)), self.max_hits, C.byref(n)))
        return det[:n.value].copy()

    # ---- parity taps
    def set_nms(self, params):
        """params: capi.NmsParams (capi.make_nms) or None.  From the next detect()/run() on, detections() and
        export_detections() return the survivors of bbNms (+ prune), in score order."""
        self._nms_keep = params
        self._chk(self.lib.acf_hip_set_nms(self.ctx, C.byref(params) if params is not None else None))

    def op_nms(self, boxes, scores, params):
        """bbNms + prune of one host list: boxes int32 [n][4] = x, y, w, h; scores float64 [n] -> indices of the survivors in order."""
        boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        n = len(scores)
        keep = np.zeros(max(n, 1), np.int32)
        cnt = C.c_int(0)
        self._chk(self.lib.acf_hip_op_nms(self.ctx, boxes.ctypes.data_as(C.POINTER(C.c_int32)), scores.ctypes.data_as(C.POINTER(C.c_double)), n,
                                          C.byref(params), keep.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(cnt)))
        return keep[:cnt.value].copy()

    def lambdas(self, frame=0):
        """The three lambdas frame `frame` of the last pyramid was approximated with (the model's, or estimated from the image)."""
        out = (C.c_double * 3)()
        self._chk(self.lib.acf_hip_get_lambdas(self.ctx, frame, out))
        return [out[0], out[1], out[2]]

    def read_level(self, frame, level):
        l = self.levels[level]
        out = np.zeros((self.nChns, l.wP, l.hP), dtype=np.float32)
        self._chk(self.lib.acf_hip_read_level(self.ctx, frame, level, capi.fptr(out)))
        return out

    def read_rank_level(self, frame, level):
        """The 16-bit threshold-rank cells of one level, as the cascade read them (after detect()/run())."""
        l = self.levels[level]
        out = np.zeros((self.nChns, l.wP, l.hP), dtype=np.uint16)
        self._chk(self.lib.acf_hip_read_rank_level(self.ctx, frame, level, out.ctypes.data_as(C.POINTER(C.c_uint16))))
        return out

    def read_pyramid(self, frame):
        return np.concatenate([self.read_level(frame, i).ravel() for i in range(len(self.levels))])

    def read_tap(self, frame, tap, index, shape):
        out = np.zeros(shape, dtype=np.float32)
        self._chk(self.lib.acf_hip_read_tap(self.ctx, frame, tap, index, capi.fptr(out), out.size))
        return out

    # ---- single operators (host planes in, host planes out)
    def op_rgb_convert(self, a, flag):
        a = np.ascontiguousarray(a, dtype=np.float32)
        _, w, h = a.shape
        out = np.zeros((1 if flag == capi.CS_GRAY else 3, w, h), dtype=np.float32)
        self._chk(self.lib.acf_hip_op_rgb_convert(self.ctx, capi.fptr(a), capi.fptr(out), h, w, flag))
        return out

    def op_conv_tri(self, a, r, aliased=True):
        a = np.ascontiguousarray(a, dtype=np.float32)
        d, w, h = a.shape
        out = np.zeros_like(a)
        self._chk(self.lib.acf_hip_op_conv_tri(self.ctx, capi.fptr(a), capi.fptr(out), h, w, d, float(r), int(aliased)))
        return out

    def op_gradient_mag(self, a, normRad=0, normConst=0.005, full=0):
        a = np.ascontiguousarray(a, dtype=np.float32)
        w, h = a.shape
        M, O, S = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
        self._chk(self.lib.acf_hip_op_gradient_mag(self.ctx, capi.fptr(a), capi.fptr(M), capi.fptr(O), capi.fptr(S), h, w, normRad, normConst, full))
        return M, O, S

    def chns_compute(self, a, model=None):
        """Detector::chnsCompute: a = host planes [d][w][h]; model = a dict like synth.make_model's (its Chns fields are read) or
        None for the context's model.  Returns [nChns][w / shrink][h / shrink]."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        d, w, h = a.shape
        pp, keep = (None, None)
        if model is not None:
            prm, keep = capi.make_params(model)
            pp = C.byref(prm)
        n, hc, wc = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.acf_hip_chns_compute(self.ctx, pp, capi.fptr(a), h, w, d, None, 0, C.byref(n), C.byref(hc), C.byref(wc)))
        out = np.zeros((n.value, wc.value, hc.value), np.float32)
        self._chk(self.lib.acf_hip_chns_compute(self.ctx, pp, capi.fptr(a), h, w, d, capi.fptr(out), out.size, C.byref(n), C.byref(hc), C.byref(wc)))
        return out

    def op_gradient_hist(self, M, O, bin=4, nOrients=6, full=0, softBin=0):
        M = np.ascontiguousarray(M, dtype=np.float32)
        O = np.ascontiguousarray(O, dtype=np.float32)
        w, h = M.shape
        H = np.zeros((nOrients, w // bin, h // bin), dtype=np.float32)
        self._chk(self.lib.acf_hip_op_gradient_hist(self.ctx, capi.fptr(M), capi.fptr(O), capi.fptr(H), h, w, bin, nOrients, softBin, full))
        return H

    def op_im_resample(self, a, hb, wb, nrm=1.0):
        a = np.ascontiguousarray(a, dtype=np.float32)
        d, wa, ha = a.shape
        out = np.zeros((d, wb, hb), dtype=np.float32)
        self._chk(self.lib.acf_hip_op_im_resample(self.ctx, capi.fptr(a), capi.fptr(out), ha, wa, hb, wb, d, float(nrm)))
        return out

    def op_im_resample_pair(self, a, hbA, wbA, hbB, wbB, nrm=1.0):
        """Two resamples of one source through k_resample_strip's two-output form (acf_hip_op_im_resample_pair, tests only) ->
        (outA, outB, dict(pair = it was launched, why = the STRIP_WHY name of the pair plan's refusal or None, slow, nty, nty_b, n_split,
        n_steps, n_steps_b of the launch))."""
        a = np.ascontiguousarray(a, dtype=np.float32)
        d, wa, ha = a.shape
        outA = np.zeros((d, wbA, hbA), dtype=np.float32)
        outB = np.zeros((d, wbB, hbB), dtype=np.float32)
        word = C.c_uint64()
        self._chk(self.lib.acf_hip_op_im_resample_pair(self.ctx, capi.fptr(a), capi.fptr(outA), capi.fptr(outB), ha, wa, hbA, wbA, hbB, wbB, d, float(nrm),
                                                       C.byref(word)))
        w = int(word.value)
        return outA, outB, dict(pair=(w & 15) == 0 and (w >> 8 & 255) > 0, why=self.STRIP_WHY[w & 15], slow=bool(w >> 4 & 1), nty=w >> 8 & 255,
                                nty_b=w >> 16 & 255, n_split=w >> 24 & 255, n_steps=w >> 32 & 0xffff, n_steps_b=w >> 48 & 0xffff)

    def op_acf_detect1(self, chns, cap=1 << 16):
        chns = np.ascontiguousarray(chns, dtype=np.float32)
        nC, wP, hP = chns.shape
        hits = np.zeros(cap, dtype=capi.HIT_DTYPE)
        n = C.c_int()
        self._chk(self.lib.acf_hip_op_acf_detect1(self.ctx, capi.fptr(chns), hP, wP, nC, hits.ctypes.data_as(C.POINTER(capi.Hit)), cap, C.byref(n)))
        return hits[:n.value].copy()

    def op_acf_detect1_rank(self, chns, cap=1 << 16):
        """op_acf_detect1 with rank cells standing for the floats (acf_hip_op_acf_detect1_rank, tests only); HipError (unsupported) where
        the call would not read rank cells."""
        chns = np.ascontiguousarray(chns, dtype=np.float32)
        nC, wP, hP = chns.shape
        hits = np.zeros(cap, dtype=capi.HIT_DTYPE)
        n = C.c_int()
        self._chk(self.lib.acf_hip_op_acf_detect1_rank(self.ctx, capi.fptr(chns), hP, wP, nC, hits.ctypes.data_as(C.POINTER(capi.Hit)), cap, C.byref(n)))
        return hits[:n.value].copy()

    def op_acf_detect1_u8(self, chns, thrs_u8=None, cap=1 << 16):
        """uint8 channel planes [nC][wP][hP]; thrs_u8 None: derived from the model's thrs (ACFIOArchive.h:96-99)."""
        chns = np.ascontiguousarray(chns, dtype=np.uint8)
        nC, wP, hP = chns.shape
        hits = np.zeros(cap, dtype=capi.HIT_DTYPE)
        n = C.c_int()
        t = None if thrs_u8 is None else np.ascontiguousarray(thrs_u8, dtype=np.uint8)
        self._chk(self.lib.acf_hip_op_acf_detect1_u8(self.ctx, chns.ctypes.data, hP, wP, nC, None if t is None else t.ctypes.data,
                                                     hits.ctypes.data_as(C.POINTER(capi.Hit)), cap, C.byref(n)))
        return hits[:n.value].copy()

    def op_evaluate(self, chns, cascThr=0.0):
        """Detector::evaluate: score of the window at (0, 0) of [nC][wP][hP] channels (acfDetect1.cpp:337-342)."""
        chns = np.ascontiguousarray(chns, dtype=np.float32)
        nC, wP, hP = chns.shape
        out = np.zeros(1, np.float32)
        self._chk(self.lib.acf_hip_op_evaluate(self.ctx, capi.fptr(chns), hP, wP, nC, float(cascThr), capi.fptr(out)))
        return out[0]

    # ---- Detector::evaluate(const cv::Mat&) for a batch of crops (device in, device out; no plan)
    def _params_of(self, chns):
        if chns is None:
            return None, None
        prm, keep = capi.make_params(chns)
        return C.byref(prm), (prm, keep)

    @staticmethod
    def _to_device(x, dtype):
        import torch
        if isinstance(x, np.ndarray):
            return torch.from_numpy(np.array(x, dtype=dtype, order="C")).cuda()
        return x

    def evaluate_crops(self, crops, chns=None, cascThr=0.0):
        """crops: float32 [n][d][w][h] (numpy, or a torch CUDA tensor), d = 1 or 3; chns: a dict like synth.make_model's whose Chns
        fields are read, or None for the context's model.  Returns the scores, float32 [n] (acf_hip_evaluate_crops)."""
        import torch
        t = self._to_device(crops, np.float32)
        n, d, w, h = t.shape
        out = torch.empty(max(n, 1), dtype=torch.float32, device=t.device)
        pp, keep = self._params_of(chns)
        self._chk(self.lib.acf_hip_evaluate_crops(self.ctx, pp, C.c_void_p(_dev_ptr(t) if n else 0), n, h, w, d, float(cascThr), C.c_void_p(out.data_ptr())))
        self.synchronize()
        return out[:n].cpu().numpy()

    def evaluate_crops_u8(self, crops, pix, row_stride=0, chns=None, cascThr=0.0, h=None, w=None):
        """crops: uint8 [n][h][w][cpp] ([n][h][w] for PIX_GRAY), or — with padded rows — [n][h * row_stride] with h and w given; numpy
        or a torch CUDA tensor.  Returns the scores, float32 [n] (acf_hip_evaluate_crops_u8)."""
        import torch
        t = self._to_device(crops, np.uint8)
        n = t.shape[0]
        if h is None or w is None:
            h, w = t.shape[1], t.shape[2]
        out = torch.empty(max(n, 1), dtype=torch.float32, device=t.device)
        pp, keep = self._params_of(chns)
        self._chk(self.lib.acf_hip_evaluate_crops_u8(self.ctx, pp, C.c_void_p(_dev_ptr_u8(t) if n else 0), n, h, w, pix, row_stride, float(cascThr),
                                                     C.c_void_p(out.data_ptr())))
        self.synchronize()
        return out[:n].cpu().numpy()


class DetectorPool:
    """N detector contexts on one GPU, each with its own HIP stream, plan and buffers; batches are handed to them in turn.

    The reference runs one acf::Detector per thread (src/app/acf/acf.cpp:255-320); here the unit is a stream.  The hot
    path alternates HBM-bound kernels (smoothing, gradMag, running sums) and VALU/LDS-bound ones (level chains, cascade), so
    independent streams let one batch's cascade run while another batch's pyramid waits on memory: 3 contexts x 96 frames
    measure +16 % over one context x 256 frames on an MI355X (profiles/ubench/two_contexts.py).
    """

    def __init__(self, n, model, H, W, d_in=3, max_batch=1, max_hits=4096, device=0, shared_device=True, **kw):
        """shared_device (default on, n > 1 only): the contexts' kernel forms are chosen for the least total work because other
        contexts' kernels fill the machine meanwhile (uncut smoothing chains, convTri's x pass on the gradient plane's chain for
        batches >= 64 frames): +4.3 % frames/s when the contexts really run side by side, -7 % when they do not — a pool that is
        fed one context at a time with a synchronise between batches should pass shared_device=False."""
        import torch
        self.streams = [torch.cuda.Stream(device=torch.device("cuda", device)) for _ in range(n)]
        self.dets = [HipDetector(model, H, W, d_in, max_batch=max_batch, max_hits=max_hits, device=device, stream=s.cuda_stream, **kw)
                     for s in self.streams]
        if n > 1:
            # the contexts' level and tile kernels (VALU / LDS-bound) take turns, so that each runs beside the other contexts'
            # memory-bound pyramid kernels and not beside another of its kind (acf_hip.h, option cascade_turns): +4 % frames/s
            # and the tile kernel runs one workgroup per tile: persistent workgroups hold every CU's LDS for the whole kernel and
            # keep the other contexts' kernels out (3 contexts: 14.0k against 13.4k frames/s; alone it is the other way round)
            # and kernel forms are chosen for the least work, not the shortest time alone (option shared_device: the smoothing chains
            # uncut, convTri's x pass on the gradient plane's chain; 3 contexts x 96 frames: +4.3 % frames/s)
            for d in self.dets:
                d.set_option("cascade_turns", 5)
                d.set_option("tile_persist", 0)
                d.set_option("shared_device", 1 if shared_device else 0)

    def __len__(self):
        return len(self.dets)

    def __iter__(self):
        return iter(zip(self.dets, self.streams))

    def synchronize(self):
        for d in self.dets:
            d.synchronize()

    def close(self):
        for d in self.dets:
            d.close()
