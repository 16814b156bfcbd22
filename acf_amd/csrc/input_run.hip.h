// input_run.hip.h — part of acf_hip.hip (included there and nowhere else): where a call's frames come from.  Every entry that takes frames
// describes them as ONE FrameSource (acf_hip.hip, beside the context, whose stream keeps the one it was opened with).  Every exported
// image / YUV entry is a one-line call of the general entry of its kind (imageEntry, yuvEntry; the streams: streamOpenYuv in acf_hip.hip)
// that fills in what it states; no exported entry calls another.  The checks stand once, in two layers: sourceArgsBad (what the call
// states, whatever the context) and sourceAgainstPlan (what the plan must be for).  planIngest decides the call's ingest once
// (IngestPlan: the preludes, the kernel, its arguments, its names) from the FrameSource's fields alone — so orient 0, scale 0 and the
// default format are the plain kernels under the plain names through whichever entry they came — and PyramidRun::ingest
// (pyramid_run.hip.h) launches that plan straight-line.  A new kind of input is one more SourceKind.
//
//   u8Geom, imageDescBad, yuvDescBad, yuvExtent      what a layout or a description is, by itself
//   videoFormatBad, video16DescBad, yuvCoef          what an acf_hip_yuv_format is, by itself: its checks and the conversion's constants
//   the kernel tables and form choosers              ingestKernel .. orientedResizedKernel, yuv16Kernel, imageLoadForm, yuvLoadForm, yuv16LoadForm, yuvIsSemiPlanar,
//                                                    yuvIsAlignedPairs, orientSrc, orientedResizedBand
//   launchYuvToRgb, launchResizeU8, launchColour     the preludes and the colour conversion (ops.hip.h and crops_run.hip.h call them too)
//   installResizeTables, resizedTables               the tap tables of acf_hip_set_input_resize (c->rz) and of the reduced sources (c->rzIn)
//   sourceArgsBad, sourceAgainstPlan                 the two layers of the checks
//   planIngest                                       FrameSource -> IngestPlan, or the refusal: planU8, planImage, planYuv, planView; planReduced, planOrientedResized
//   imageEntry, yuvEntry and the exported entries    acf_hip_pyramid_u8 / _image* / _yuv* / _video and their run_ twins, the extents and layouts,
//                                                    acf_hip_set_yuv_layout, acf_hip_set_input_resize, acf_hip_yuv_to_rgb8 / video_to_rgb (videoToRgb)
//   viewEntry and the view entries                   acf_hip_pyramid_view / acf_hip_run_view (SRC_VIEW: affine views of stored frames, k_ingest_view) and their host
//                                                    arithmetic acf_hip_view_from_box / _view_quad / _view_box / _view_form
#pragma once

namespace
{
int pyramidImpl(acf_hip_ctx* c, const FrameSource& src, int nF); // (acf_hip.hip, behind pyramid_run.hip.h)

using IngestKernel = void (*)(IngestArgs);
using YuvIngestKernel = void (*)(IngestArgs, YuvSrc);
using ImageKernel = void (*)(IngestArgs, ImageArgs);
using YuvDescKernel = void (*)(IngestArgs, YuvDescSrc);
using ResizedKernel = void (*)(IngestArgs, ResizedSrc);
using ImageOrientedKernel = void (*)(IngestArgs, ImageOrientedSrc);
using YuvOrientedKernel = void (*)(IngestArgs, YuvOrientedSrc);
using OrientedResizedKernel = void (*)(IngestArgs, OrientedResizedSrc);
using Yuv16Kernel = void (*)(IngestArgs, Yuv16Src);
using ViewKernel = void (*)(IngestArgs, ViewSrc);

static IngestKernel ingestKernel(int mode, bool aligned)
{
    switch (mode)
    {
        case IG_LUV_VEC: return aligned ? k_ingest_u8<IG_LUV_VEC, true> : k_ingest_u8<IG_LUV_VEC, false>;
        case IG_LUV: return aligned ? k_ingest_u8<IG_LUV, true> : k_ingest_u8<IG_LUV, false>;
        case IG_GRAY: return aligned ? k_ingest_u8<IG_GRAY, true> : k_ingest_u8<IG_GRAY, false>;
        default: return aligned ? k_ingest_u8<IG_PLANAR, true> : k_ingest_u8<IG_PLANAR, false>;
    }
}

// (no IG_LUV: a YUV 4:2:0 frame has even H and W, so H * W % 4 == 0 and rgbConvert takes the vector body, rgbConvertMex.cpp:92,343)
static YuvIngestKernel yuvIngestKernel(int mode, bool aligned, bool cf = false)
{
    if (cf) // a format other than the default: the constants from YuvSrc::k
    {
        switch (mode)
        {
            case IG_LUV_VEC: return aligned ? k_ingest_yuv420<IG_LUV_VEC, true, true> : k_ingest_yuv420<IG_LUV_VEC, false, true>;
            case IG_GRAY: return aligned ? k_ingest_yuv420<IG_GRAY, true, true> : k_ingest_yuv420<IG_GRAY, false, true>;
            default: return aligned ? k_ingest_yuv420<IG_PLANAR, true, true> : k_ingest_yuv420<IG_PLANAR, false, true>;
        }
    }
    switch (mode)
    {
        case IG_LUV_VEC: return aligned ? k_ingest_yuv420<IG_LUV_VEC, true> : k_ingest_yuv420<IG_LUV_VEC, false>;
        case IG_GRAY: return aligned ? k_ingest_yuv420<IG_GRAY, true> : k_ingest_yuv420<IG_GRAY, false>;
        default: return aligned ? k_ingest_yuv420<IG_PLANAR, true> : k_ingest_yuv420<IG_PLANAR, false>;
    }
}

// k_ingest_image<element type, conversion>: [ACF_HIP_T_*][IG_*]
static ImageKernel imageKernel(int dtype, int mode)
{
    static const ImageKernel table[4][4] = {
        { k_ingest_image<IM_U8, IG_PLANAR>, k_ingest_image<IM_U8, IG_LUV_VEC>, k_ingest_image<IM_U8, IG_LUV>, k_ingest_image<IM_U8, IG_GRAY> },
        { k_ingest_image<IM_F16, IG_PLANAR>, k_ingest_image<IM_F16, IG_LUV_VEC>, k_ingest_image<IM_F16, IG_LUV>, k_ingest_image<IM_F16, IG_GRAY> },
        { k_ingest_image<IM_BF16, IG_PLANAR>, k_ingest_image<IM_BF16, IG_LUV_VEC>, k_ingest_image<IM_BF16, IG_LUV>, k_ingest_image<IM_BF16, IG_GRAY> },
        { k_ingest_image<IM_F32, IG_PLANAR>, k_ingest_image<IM_F32, IG_LUV_VEC>, k_ingest_image<IM_F32, IG_LUV>, k_ingest_image<IM_F32, IG_GRAY> },
    };
    return table[dtype][mode];
}

// k_ingest_yuv<conversion, load form, constants as an argument>: [cf][YD_*][IG_*]
static YuvDescKernel yuvDescKernel(int form, int mode, bool cf = false)
{
#define YDK(FORM, CF) { k_ingest_yuv<IG_PLANAR, FORM, CF>, k_ingest_yuv<IG_LUV_VEC, FORM, CF>, k_ingest_yuv<IG_LUV, FORM, CF>, k_ingest_yuv<IG_GRAY, FORM, CF> }
    static const YuvDescKernel table[2][3][4] = { { YDK(YD_GENERIC, false), YDK(YD_PLANAR, false), YDK(YD_PACKED422, false) },
        { YDK(YD_GENERIC, true), YDK(YD_PLANAR, true), YDK(YD_PACKED422, true) } };
#undef YDK
    return table[cf][form][mode];
}

// k_ingest_yuv16<conversion, load form>: [YD16_*][IG_*]
static Yuv16Kernel yuv16Kernel(int form, int mode)
{
#define Y16K(FORM) { k_ingest_yuv16<IG_PLANAR, FORM>, k_ingest_yuv16<IG_LUV_VEC, FORM>, k_ingest_yuv16<IG_LUV, FORM>, k_ingest_yuv16<IG_GRAY, FORM> }
    static const Yuv16Kernel table[3][4] = { Y16K(YD16_GENERIC), Y16K(YD16_PLANAR), Y16K(YD16_PAIRS) };
#undef Y16K
    return table[form][mode];
}

// k_ingest_resized<source, conversion>: [RS_*][IG_*]
static ResizedKernel resizedKernel(int src, int mode)
{
    static const ResizedKernel table[3][4] = {
        { k_ingest_resized<RS_IMAGE, IG_PLANAR>, k_ingest_resized<RS_IMAGE, IG_LUV_VEC>, k_ingest_resized<RS_IMAGE, IG_LUV>, k_ingest_resized<RS_IMAGE, IG_GRAY> },
        { k_ingest_resized<RS_YUV, IG_PLANAR>, k_ingest_resized<RS_YUV, IG_LUV_VEC>, k_ingest_resized<RS_YUV, IG_LUV>, k_ingest_resized<RS_YUV, IG_GRAY> },
        { k_ingest_resized<RS_YUV_CF, IG_PLANAR>, k_ingest_resized<RS_YUV_CF, IG_LUV_VEC>, k_ingest_resized<RS_YUV_CF, IG_LUV>, k_ingest_resized<RS_YUV_CF, IG_GRAY> },
    };
    return table[src][mode];
}

// k_ingest_image_oriented<element type, conversion>: [ACF_HIP_T_*][IG_*] (the load form and the orientation are arguments)
static ImageOrientedKernel imageOrientedKernel(int dtype, int mode)
{
    static const ImageOrientedKernel table[4][4] = {
        { k_ingest_image_oriented<IM_U8, IG_PLANAR>, k_ingest_image_oriented<IM_U8, IG_LUV_VEC>, k_ingest_image_oriented<IM_U8, IG_LUV>,
            k_ingest_image_oriented<IM_U8, IG_GRAY> },
        { k_ingest_image_oriented<IM_F16, IG_PLANAR>, k_ingest_image_oriented<IM_F16, IG_LUV_VEC>, k_ingest_image_oriented<IM_F16, IG_LUV>,
            k_ingest_image_oriented<IM_F16, IG_GRAY> },
        { k_ingest_image_oriented<IM_BF16, IG_PLANAR>, k_ingest_image_oriented<IM_BF16, IG_LUV_VEC>, k_ingest_image_oriented<IM_BF16, IG_LUV>,
            k_ingest_image_oriented<IM_BF16, IG_GRAY> },
        { k_ingest_image_oriented<IM_F32, IG_PLANAR>, k_ingest_image_oriented<IM_F32, IG_LUV_VEC>, k_ingest_image_oriented<IM_F32, IG_LUV>,
            k_ingest_image_oriented<IM_F32, IG_GRAY> },
    };
    return table[dtype][mode];
}

// k_ingest_yuv_oriented<conversion, constants as an argument>: [cf][IG_*]
static YuvOrientedKernel yuvOrientedKernel(int mode, bool cf = false)
{
    static const YuvOrientedKernel table[2][4] = { { k_ingest_yuv_oriented<IG_PLANAR>, k_ingest_yuv_oriented<IG_LUV_VEC>, k_ingest_yuv_oriented<IG_LUV>,
                                                       k_ingest_yuv_oriented<IG_GRAY> },
        { k_ingest_yuv_oriented<IG_PLANAR, true>, k_ingest_yuv_oriented<IG_LUV_VEC, true>, k_ingest_yuv_oriented<IG_LUV, true>, k_ingest_yuv_oriented<IG_GRAY, true> } };
    return table[cf][mode];
}

// k_ingest_oriented_resized<source, conversion, staged>: [RS_*][IG_*], the LDS-staged form or the global gather
static OrientedResizedKernel orientedResizedKernel(int src, int mode, bool staged)
{
#define ORK(SRC, ST) { k_ingest_oriented_resized<SRC, IG_PLANAR, ST>, k_ingest_oriented_resized<SRC, IG_LUV_VEC, ST>, k_ingest_oriented_resized<SRC, IG_LUV, ST>, \
                       k_ingest_oriented_resized<SRC, IG_GRAY, ST> }
    static const OrientedResizedKernel table[2][3][4] = { { ORK(RS_IMAGE, false), ORK(RS_YUV, false), ORK(RS_YUV_CF, false) },
        { ORK(RS_IMAGE, true), ORK(RS_YUV, true), ORK(RS_YUV_CF, true) } };
#undef ORK
    return table[staged][src][mode];
}

// k_ingest_view<source kind, conversion>: [CUT_*][IG_*] (the form is decided per tile, in the kernel)
static ViewKernel viewKernel(int kind, int mode)
{
#define VK(KIND) { k_ingest_view<KIND, IG_PLANAR>, k_ingest_view<KIND, IG_LUV_VEC>, k_ingest_view<KIND, IG_LUV>, k_ingest_view<KIND, IG_GRAY> }
    static const ViewKernel table[7][4] = { VK(CUT_IMG_U8), VK(CUT_IMG_F16), VK(CUT_IMG_BF16), VK(CUT_IMG_F32), VK(CUT_YUV8), VK(CUT_YUV8_CF), VK(CUT_YUV16) };
#undef VK
    return table[kind][mode];
}

static bool pixIsYuv(int pix)
{
    return pix == ACF_HIP_PIX_NV12 || pix == ACF_HIP_PIX_NV21;
}

// Where the bytes of a batch of 8-bit frames of rows x cols lie — the ONE place that knows (acf_hip_u8_frame_bytes, the ingest, the
// input resize, the stream's buffers).  rowStride 0 = tight.  NV12 / NV21: cpp = 1 (the luma plane); chromaOff / frameStride are
// acf_hip_set_yuv_layout's (0 = tight: chroma behind the luma rows, frames stride * rows * 3 / 2 apart).  The packed layouts have
// no such freedom: frames are stride * rows apart.  Returns what is wrong, or null.
struct U8Geom
{
    int cpp, stride;
    int ro, go, bo; // byte offsets of r, g, b inside a packed pixel
    bool yuv;
    int64_t chromaOff, frameStride;
};
static const char* u8Geom(int pix, int rows, int cols, int rowStride, int64_t chromaOff, int64_t frameStride, U8Geom& g)
{
    g = U8Geom{};
    switch (pix)
    {
        case ACF_HIP_PIX_RGB: g.cpp = 3, g.ro = 0, g.go = 1, g.bo = 2; break;
        case ACF_HIP_PIX_BGR: g.cpp = 3, g.ro = 2, g.go = 1, g.bo = 0; break;
        case ACF_HIP_PIX_RGBA: g.cpp = 4, g.ro = 0, g.go = 1, g.bo = 2; break;
        case ACF_HIP_PIX_BGRA: g.cpp = 4, g.ro = 2, g.go = 1, g.bo = 0; break;
        case ACF_HIP_PIX_GRAY: g.cpp = 1; break;
        case ACF_HIP_PIX_NV12:
        case ACF_HIP_PIX_NV21: g.cpp = 1, g.yuv = true; break;
        default: return "pixel layout";
    }
    if (rows < 1 || cols < 1 || rowStride < 0)
    {
        return "frame size";
    }
    if (int64_t(cols) * g.cpp > INT32_MAX)
    {
        return "frame size";
    }
    g.stride = rowStride > 0 ? rowStride : cols * g.cpp;
    if (g.stride < cols * g.cpp)
    {
        return "row stride smaller than a row";
    }
    const int64_t plane = int64_t(g.stride) * rows;
    if (!g.yuv)
    {
        g.frameStride = plane;
        return nullptr;
    }
    if (rows % 2 || cols % 2)
    {
        return "NV12 / NV21 frames have even rows and columns";
    }
    g.chromaOff = chromaOff > 0 ? chromaOff : plane;
    if (g.chromaOff < plane)
    {
        return "chroma offset inside the luma plane";
    }
    g.frameStride = frameStride > 0 ? frameStride : g.chromaOff + plane / 2;
    if (g.frameStride < g.chromaOff + plane / 2)
    {
        return "frame stride smaller than a frame (frames would overlap)";
    }
    return nullptr;
}

// the plan's input planes against the layout: 1 for GRAY, 3 for the colour layouts — NV12 / NV21 included: the luma plane is limited
// range, not the grey cvtColor gives, so a 1-plane plan does not take it
static bool u8PlanesOk(const U8Geom& g, int d_in)
{
    return (g.cpp == 1 && !g.yuv) == (d_in == 1);
}

static YuvSrc yuvSrc(const uint8_t* frames, int pix, int rows, int cols, const U8Geom& g)
{
    YuvSrc s{};
    s.in = frames;
    s.H = rows;
    s.W = cols;
    s.rowStride = g.stride;
    s.vFirst = pix == ACF_HIP_PIX_NV21;
    s.chromaOff = g.chromaOff;
    s.in_fs = g.frameStride;
    return s;
}

// k_yuv420_to_rgb8 over a batch: NV12 / NV21 frames of rows x cols -> tight RGB frames at dst
static int launchYuvToRgb(acf_hip_ctx* c, const YuvSrc& s, int nF, uint8_t* dst)
{
    prof(c, c->stream, "k_yuv420_to_rgb8");
    hipLaunchKernelGGL(k_yuv420_to_rgb8, dim3(cdiv(s.W / 2, 64), cdiv(s.H / 2, 4), nF), dim3(256), 0, c->stream, s, dst);
    LAUNCHCHK(c, "k_yuv420_to_rgb8");
    return ACF_HIP_OK;
}

// The conversion an ingest kernel does on its way (IG_*).  convert: to the converted colour planes; else planar, the input's own planes.
static int ingestMode(const acf_hip_ctx* c, bool convert)
{
    if (convert && c->p.colorSpace == ACF_HIP_CS_LUV)
    {
        return (int64_t(c->plan.H) * c->plan.W % 4 == 0) ? IG_LUV_VEC : IG_LUV; // rgbConvertMex.cpp:92,343
    }
    if (convert && c->p.colorSpace == ACF_HIP_CS_GRAY)
    {
        return IG_GRAY; // a 1-plane input is replicated first (chnsPyramid.cpp:234-244): r == g == b
    }
    return IG_PLANAR;
}

// What every ingest kernel is told, whatever it reads: the nOut destination planes and the constants of the model's colour conversion
static void ingestShared(acf_hip_ctx* c, float* dst, int64_t out_fs, int nOut, IngestArgs& a)
{
    const Plan& pl = c->plan;
    a.out = dst;
    a.nOut = nOut;
    a.lTable = c->d_lTable;
    a.k = makeLuvConsts();
    a.x86 = x86T(c);
    a.mr = kGray.r;
    a.mg = kGray.g;
    a.mb = kGray.b;
    a.H = pl.H;
    a.W = pl.W;
    a.out_fs = out_fs;
    a.vecStore = (pl.H % 4 == 0) && (out_fs % 4 == 0) && (reinterpret_cast<uintptr_t>(dst) % 16 == 0);
}

// What is wrong with an image description by itself (acf_hip_image_extent and the image entries), or null
static const char* imageDescBad(const acf_hip_image_desc* d)
{
    if (!d)
    {
        return "null description";
    }
    if (d->dtype < ACF_HIP_T_U8 || d->dtype > ACF_HIP_T_F32)
    {
        return "unknown dtype";
    }
    if (d->channels != 1 && d->channels != 3)
    {
        return "channels must be 1 or 3";
    }
    if (d->stride_x < 1 || d->stride_y < 1)
    {
        return "stride_x and stride_y must be positive";
    }
    if (d->stride_n < 0)
    {
        return "negative stride_n";
    }
    return nullptr;
}

static int imageElemBytes(int dtype)
{
    return dtype == ACF_HIP_T_U8 ? 1 : (dtype == ACF_HIP_T_F32 ? 4 : 2);
}

// an image description as the kernels take it (without the load form)
static ImageArgs imageArgs(const void* frames, const acf_hip_image_desc& d)
{
    ImageArgs s{};
    s.in = frames;
    s.sn = d.stride_n;
    s.sc = d.stride_c;
    s.sy = d.stride_y;
    s.sx = d.stride_x;
    s.nIn = d.channels;
    return s;
}

// The load form of k_ingest_image for a description and a pointer: the vector forms where their conditions hold (kernels_input.hip.h),
// else the element-wise one, which is right for every description.
static int imageLoadForm(const void* frames, const acf_hip_image_desc& d)
{
    const uintptr_t at = reinterpret_cast<uintptr_t>(frames);
    const int es = imageElemBytes(d.dtype);
    if (at % es)
    {
        return IM_GENERIC;
    }
    if (d.stride_x == 1 && at % (4 * es) == 0 && d.stride_n % 4 == 0 && d.stride_y % 4 == 0 && (d.channels == 1 || d.stride_c % 4 == 0))
    {
        return IM_ROWVEC;
    }
    if (d.channels == 3 && (d.stride_c == 1 || d.stride_c == -1) && (d.stride_x == 3 || d.stride_x == 4))
    {
        return IM_PACKED;
    }
    return IM_GENERIC;
}

// What is wrong with a YUV description by itself (acf_hip_yuv_extent, the YUV entries), or null
static const char* yuvDescBad(const acf_hip_yuv_desc* d)
{
    if (!d)
    {
        return "null description";
    }
    if (d->sub_x < 0 || d->sub_x > 1 || d->sub_y < 0 || d->sub_y > 1)
    {
        return "sub_x and sub_y must be 0 or 1";
    }
    for (const acf_hip_yuv_plane* p : { &d->y, &d->u, &d->v })
    {
        if (p->stride_px < 1 || p->stride_row < 1)
        {
            return "stride_px and stride_row must be positive";
        }
        if (p->stride_n < 0)
        {
            return "negative stride_n";
        }
    }
    return nullptr;
}

// first / last byte offset plane by plane (Y, U, V) that nF frames of h x w address
static void yuvExtent(const acf_hip_yuv_desc& d, int h, int w, int nF, int64_t first[3], int64_t last[3])
{
    const acf_hip_yuv_plane* pl[3] = { &d.y, &d.u, &d.v };
    for (int i = 0; i < 3; i++)
    {
        const int rows = i ? (h + d.sub_y) >> d.sub_y : h, cols = i ? (w + d.sub_x) >> d.sub_x : w;
        first[i] = pl[i]->offset; // (no stride is negative)
        last[i] = pl[i]->offset + int64_t(nF - 1) * pl[i]->stride_n + int64_t(rows - 1) * pl[i]->stride_row + int64_t(cols - 1) * pl[i]->stride_px;
    }
}

// The default format: the arithmetic of the YUV entries ({8, 0, BT601, 0}; a null format is it)
static const acf_hip_yuv_format kDefaultVideoFormat{ 8, 0, ACF_HIP_YUV_MATRIX_BT601, 0 };
static bool videoFormatIsDefault(const acf_hip_yuv_format& f)
{
    return f.bits == 8 && f.shift == 0 && f.matrix == ACF_HIP_YUV_MATRIX_BT601 && f.full_range == 0;
}

// What is wrong with a format by itself, or null
static const char* videoFormatBad(const acf_hip_yuv_format& f)
{
    if (f.bits < 8 || f.bits > 16)
    {
        return "bits must be 8 .. 16";
    }
    if (f.shift < 0 || (f.bits == 8 && f.shift != 0) || f.shift + f.bits > 16)
    {
        return "shift must be 0 for 8 bits, and shift + bits <= 16";
    }
    if (f.matrix < ACF_HIP_YUV_MATRIX_BT601 || f.matrix > ACF_HIP_YUV_MATRIX_BT2020)
    {
        return "unknown matrix (ACF_HIP_YUV_MATRIX_*)";
    }
    if (f.full_range != 0 && f.full_range != 1)
    {
        return "full_range must be 0 or 1";
    }
    return nullptr;
}

// 16-bit words: what is wrong with the description (and the pointer, when there is one) for them, or null
static const char* video16DescBad(const void* base, const acf_hip_yuv_desc& d)
{
    if (reinterpret_cast<uintptr_t>(base) % 2)
    {
        return "16-bit samples need an even base";
    }
    for (const acf_hip_yuv_plane* p : { &d.y, &d.u, &d.v })
    {
        if (p->offset % 2 || p->stride_n % 2 || p->stride_row % 2 || p->stride_px % 2)
        {
            return "16-bit samples need even offsets and strides";
        }
    }
    return nullptr;
}

// The constants of a (checked) format: round(2^20 * q), half away from zero, q the exact rational from Kr / Kb with the luma gain
// 255 / 219 and the chroma gain 255 / 224 for limited range (tests/video_format_ref.py derives them again with fractions.Fraction);
// BT.601 limited keeps cvtColor's (from coefficients rounded to three decimals): yuv_chroma / yuv_rgb's own
static YuvCoef yuvCoef(const acf_hip_yuv_format& f)
{
    static const int table[3][2][5] = {
        { { 1220542, 1673527, -852492, -409993, 2116026 }, { 1048576, 1470104, -748826, -360853, 1858077 } },
        { { 1220945, 1879825, -558796, -223607, 2215014 }, { 1048576, 1651297, -490864, -196424, 1945738 } },
        { { 1220945, 1760217, -682019, -196426, 2245811 }, { 1048576, 1546230, -599107, -172546, 1972791 } },
    };
    const int* t = table[f.matrix][f.full_range];
    YuvCoef k{};
    k.yoff = f.full_range ? 0 : 16 << (f.bits - 8);
    k.cmid = 1 << (f.bits - 1);
    k.omax = f.full_range ? (1 << f.bits) - 1 : 255 << (f.bits - 8);
    k.cy = t[0];
    k.cvr = t[1];
    k.cvg = t[2];
    k.cug = t[3];
    k.cub = t[4];
    k.sc = float(1.0 / double(k.omax));
    return k;
}

static YuvDescSrc yuvDescSrc(const uint8_t* base, const acf_hip_yuv_desc& d)
{
    YuvDescSrc s{};
    s.base = base;
    s.y = YuvPlane{ d.y.offset, d.y.stride_n, d.y.stride_row, d.y.stride_px };
    s.u = YuvPlane{ d.u.offset, d.u.stride_n, d.u.stride_row, d.u.stride_px };
    s.v = YuvPlane{ d.v.offset, d.v.stride_n, d.v.stride_row, d.v.stride_px };
    s.subX = d.sub_x;
    s.subY = d.sub_y;
    return s;
}

// The load form of k_ingest_yuv for a description and a pointer: the vector forms where their conditions hold (kernels_input.hip.h),
// else the byte form, which is right for every description.  YD_PACKED422 also fills in the macropixel's byte order.
static int yuvLoadForm(YuvDescSrc& s)
{
    const uintptr_t at = reinterpret_cast<uintptr_t>(s.base);
    const auto aligned = [&](const YuvPlane& p) { return (at + uintptr_t(p.off)) % 4 == 0 && p.sr % 4 == 0 && p.sn % 4 == 0; };
    if (s.y.sp == 1 && s.u.sp == 1 && s.v.sp == 1 && aligned(s.y) && aligned(s.u) && aligned(s.v))
    {
        return YD_PLANAR;
    }
    if (s.subX == 1 && s.subY == 0 && s.y.sp == 2 && s.u.sp == 4 && s.v.sp == 4 && s.y.sr == s.u.sr && s.y.sr == s.v.sr && s.y.sn == s.u.sn &&
        s.y.sn == s.v.sn)
    {
        const int64_t mp = std::min(s.y.off, std::min(s.u.off, s.v.off));
        const int64_t yp = s.y.off - mp, up = s.u.off - mp, vp = s.v.off - mp;
        // Y0, Y1, U, V take the four bytes of one aligned macropixel
        if (yp <= 1 && up <= 3 && vp <= 3 && ((1 << yp) | (1 << (yp + 2)) | (1 << up) | (1 << vp)) == 15 && (at + uintptr_t(mp)) % 4 == 0 && s.y.sr % 4 == 0 &&
            s.y.sn % 4 == 0)
        {
            s.mp = mp;
            s.yPos = int(yp);
            s.uPos = int(up);
            s.vPos = int(vp);
            return YD_PACKED422;
        }
    }
    return YD_GENERIC;
}

// The load form of k_ingest_yuv16 for a (checked: all even) description and a pointer; YD16_PAIRS also says which word comes first
static int yuv16LoadForm(const YuvDescSrc& s, int& vFirst)
{
    const uintptr_t at = reinterpret_cast<uintptr_t>(s.base);
    const auto aligned = [&](const YuvPlane& p) { return (at + uintptr_t(p.off)) % 4 == 0 && p.sr % 4 == 0 && p.sn % 4 == 0; };
    vFirst = 0;
    if (s.y.sp != 2 || !aligned(s.y))
    {
        return YD16_GENERIC;
    }
    if (s.u.sp == 2 && s.v.sp == 2 && aligned(s.u) && aligned(s.v))
    {
        return YD16_PLANAR;
    }
    const YuvPlane& lo = s.v.off < s.u.off ? s.v : s.u;
    if (s.u.sp == 4 && s.v.sp == 4 && std::max(s.u.off, s.v.off) == lo.off + 2 && s.u.sr == s.v.sr && s.u.sn == s.v.sn && aligned(lo))
    {
        vFirst = s.v.off < s.u.off;
        return YD16_PAIRS;
    }
    return YD16_GENERIC;
}

// A description of an NV12 / NV21 frame as the 8-bit entry takes it (one row stride, interleaved chroma pairs, even sizes): the
// YuvSrc of k_ingest_yuv420, which then runs it — the same kernel, so the same bits as acf_hip_run_u8(ACF_HIP_PIX_NV12 / _NV21)
static bool yuvIsSemiPlanar(const uint8_t* base, const acf_hip_yuv_desc& d, int H, int W, YuvSrc& out)
{
    const int64_t c0 = std::min(d.u.offset, d.v.offset);
    if (!(d.sub_x == 1 && d.sub_y == 1 && H % 2 == 0 && W % 2 == 0 && d.y.stride_px == 1 && d.u.stride_px == 2 && d.v.stride_px == 2 &&
            std::max(d.u.offset, d.v.offset) == c0 + 1 && d.u.stride_row == d.y.stride_row && d.v.stride_row == d.y.stride_row && d.y.stride_row <= INT32_MAX &&
            d.u.stride_n == d.y.stride_n && d.v.stride_n == d.y.stride_n))
    {
        return false;
    }
    out = YuvSrc{};
    out.in = base + d.y.offset;
    out.H = H;
    out.W = W;
    out.rowStride = int(d.y.stride_row);
    out.vFirst = d.v.offset < d.u.offset;
    out.chromaOff = c0 - d.y.offset;
    out.in_fs = d.y.stride_n;
    return true;
}

// rgbConvert of nF frames of n pixels: `in` holds nIn planes a frame (frame stride in_fs), `out` the converted planes (out_fs).  LUV takes
// the vector body iff n % 4 == 0 (rgbConvertMex.cpp:92,343); a 1-plane input is replicated first (chnsPyramid.cpp:234-244): gray from
// it is k_rgb2gray<true>, ORIG / RGB k_replicate3.  The caller checks the launch.
static void launchColour(acf_hip_ctx* c, const float* in, float* out, int64_t n, int nF, int64_t in_fs, int64_t out_fs, int colorSpace, int nIn)
{
    const dim3 grid(cdiv(n, 256), 1, nF), block(256);
    if (colorSpace == ACF_HIP_CS_LUV)
    {
        hipLaunchKernelGGL((n % 4 == 0 ? k_rgb2luv<true> : k_rgb2luv<false>), grid, block, 0, c->stream, in, out, (const float*)c->d_lTable, makeLuvConsts(),
            int(n), in_fs, out_fs, x86T(c));
    }
    else if (colorSpace == ACF_HIP_CS_GRAY)
    {
        hipLaunchKernelGGL((nIn == 1 ? k_rgb2gray<true> : k_rgb2gray<false>), grid, block, 0, c->stream, in, out, int(n), in_fs, out_fs, kGray.r, kGray.g,
            kGray.b);
    }
    else if (colorSpace == ACF_HIP_CS_HSV)
    {
        hipLaunchKernelGGL(k_rgb2hsv, grid, block, 0, c->stream, in, out, int(n), in_fs, out_fs);
    }
    else
    {
        hipLaunchKernelGGL(k_replicate3, grid, block, 0, c->stream, in, out, int(n), in_fs, out_fs);
    }
}

// what rz_pixel reads besides the source: the tables on the device and the source size
static ResizeTaps resizeTaps(const acf_hip_ctx::InputResize& rz)
{
    ResizeTaps t{};
    t.rows = rz.t.rows;
    t.cols = rz.t.cols;
    t.mode = rz.t.mode;
    t.isx = rz.t.isx;
    t.isy = rz.t.isy;
    t.xlin = reinterpret_cast<const int4*>(rz.d_xlin);
    t.ylin = reinterpret_cast<const int4*>(rz.d_ylin);
    t.xrun = reinterpret_cast<const int2*>(rz.d_xrun);
    t.yrun = reinterpret_cast<const int2*>(rz.d_yrun);
    t.xtap = reinterpret_cast<const int2*>(rz.d_xtap);
    t.ytap = reinterpret_cast<const int2*>(rz.d_ytap);
    return t;
}

// k_resize_u8 over a batch: `src` frames of t.rows x t.cols (row stride `stride` bytes) -> tight t.drows x t.dcols frames at dst
static int launchResizeU8(acf_hip_ctx* c, const acf_hip_ctx::InputResize& rz, const uint8_t* src, int cpp, int stride, int nF, uint8_t* dst)
{
    const ResizeTables& t = rz.t;
    ResizeArgs a{};
    a.src = src;
    a.dst = dst;
    a.cn = cpp;
    a.stride = stride;
    a.drows = t.drows;
    a.dcols = t.dcols;
    a.src_fs = int64_t(stride) * t.rows;
    a.dst_fs = int64_t(t.drows) * t.dcols * cpp;
    a.t = resizeTaps(rz);
    prof(c, c->stream, "k_resize_u8");
    hipLaunchKernelGGL(k_resize_u8, dim3(cdiv(t.dcols, 64), cdiv(t.drows, 4), nF), dim3(256), 0, c->stream, a);
    LAUNCHCHK(c, "k_resize_u8");
    return ACF_HIP_OK;
}

static int uploadResizeTables(acf_hip_ctx* c, acf_hip_ctx::InputResize& rz)
{
    int rc;
    if ((rc = devUpload(c, &rz.d_xlin, rz.t.xlin)) || (rc = devUpload(c, &rz.d_ylin, rz.t.ylin)) || (rc = devUpload(c, &rz.d_xrun, rz.t.xrun)) ||
        (rc = devUpload(c, &rz.d_yrun, rz.t.yrun)) || (rc = devUpload(c, &rz.d_xtap, rz.t.xtap)) || (rc = devUpload(c, &rz.d_ytap, rz.t.ytap)))
    {
        return rc;
    }
    return ACF_HIP_OK;
}

static void releaseResize(acf_hip_ctx* c, acf_hip_ctx::InputResize& r)
{
    devRelease(c, r.d_xlin);
    devRelease(c, r.d_ylin);
    devRelease(c, r.d_xrun);
    devRelease(c, r.d_yrun);
    devRelease(c, r.d_xtap);
    devRelease(c, r.d_ytap);
    devRelease(c, r.d_out);
}

// The tap tables of (srcRows, srcCols, scale) into `slot` (c->rz or c->rzIn) in place of the ones it holds: built, held against the
// plan, uploaded — with the reduced 8-bit frames' buffer where k_resize_u8 is to run (withOut) — and installed switched on
static int installResizeTables(acf_hip_ctx* c, const char* who, acf_hip_ctx::InputResize& slot, int srcRows, int srcCols, double scale, bool withOut)
{
    acf_hip_ctx::InputResize rz;
    if (buildResizeTables(srcRows, srcCols, scale, rz.t) || rz.t.drows != c->plan.H || rz.t.dcols != c->plan.W)
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(who) + ": the plan must be for the reduced size (acf_hip_resize_dims of the frame size and scale)");
    }
    rz.rows = srcRows;
    rz.cols = srcCols;
    rz.scale = scale;
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = uploadResizeTables(c, rz)) || (withOut && (rc = devAlloc(c, &rz.d_out, size_t(c->maxBatch) * c->plan.H * c->plan.W * 4))))
    {
        releaseResize(c, rz); // (what was uploaded before the failure)
        return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream)); // the previous tables: a batch in flight may still read them
    releaseResize(c, slot);
    rz.on = true;
    slot = rz;
    return ACF_HIP_OK;
}

// every entry but the 8-bit one, while acf_hip_set_input_resize is switched on
static int inputResizeRefused(acf_hip_ctx* c, const char* who, const char* why)
{
    return fail(c, ACF_HIP_E_INVALID, std::string(who) + ": not with acf_hip_set_input_resize (" + why + ")");
}

// What the resized entries refuse about (src_rows, src_cols, scale) and the plan, then their tap tables on the device: those of the
// context's key (rows, cols, scale) as they are, else new ones
static int resizedTables(acf_hip_ctx* c, const char* who, int srcRows, int srcCols, double scale)
{
    if (srcRows < 1 || srcCols < 1 || !(scale > 0) || !std::isfinite(scale))
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(who) + ": src_rows and src_cols >= 1, scale a positive finite number");
    }
    if (c->rz.on)
    {
        return inputResizeRefused(c, who, "the entry resizes by itself");
    }
    const acf_hip_ctx::InputResize& cur = c->rzIn;
    if (cur.on && cur.rows == srcRows && cur.cols == srcCols && cur.scale == scale)
    {
        return ACF_HIP_OK; // (built against this plan: acf_hip_plan drops them)
    }
    return installResizeTables(c, who, c->rzIn, srcRows, srcCols, scale, false);
}

// An orientation code (ACF_HIP_ORIENT_*: rot + 4 * mirror) as the map from upright to source indices that the kernels and
// acf_hip_unorient_rect take (kernels_input.hip.h): rot 1: swap, revR; rot 2: revR, revC; rot 3: swap, revC; mirror flips revC
static OrientSrc orientSrc(int code, int srcRows, int srcCols)
{
    const int rot = code & 3, mirror = (code >> 2) & 1;
    OrientSrc o{};
    o.Hs = srcRows;
    o.Ws = srcCols;
    o.swap = rot & 1;
    o.revR = rot == 1 || rot == 2;
    o.revC = (rot >= 2) != (mirror != 0);
    return o;
}

// a stored frame size and an orientation code, by themselves (acf_hip_oriented_dims, acf_hip_unorient_rect and the entries that state them)
static bool orientedArgsBad(int srcRows, int srcCols, int orient)
{
    return orient < 0 || orient > 7 || srcRows < 1 || srcCols < 1;
}

// Which of (srcRows, srcCols, orient, scale) a call states beside its description: what its exported entry takes
enum Stated
{
    ST_PLAN,           // none: upright frames of the plan's size
    ST_REDUCED,        // the size and the scale; both are held together with the tap tables (resizedTables), after the description and the planes
    ST_TURNED,         // the size and the orientation
    ST_TURNED_REDUCED, // all four; the scale is held with the tap tables
    ST_VIDEO           // all four and a format, 0 meaning "none": scale 0 = no resize, everything 0 = ST_PLAN
};

// What is wrong with what a call states about its frames, whatever the context is — the first layer of the checks: the refusal, or OK
// with src.resized decided.  src holds the call's arguments (who, fmt, srcRows, srcCols, orient, scale); `who` names the entry where
// the format, the scale and the sample width are refused (run_video says its own name there, pyramid_video's everywhere else).
// open: the call is a stream's open, which has always kept an order of its own in two places (below), so that a call that is wrong
// in two ways keeps its error code.
static int sourceArgsBad(acf_hip_ctx* c, const char* who, Stated st, FrameSource& src, bool open = false)
{
    const std::string w = std::string(who) + ": ";
    bool sized = st == ST_TURNED || st == ST_TURNED_REDUCED, wide = false;
    src.resized = st == ST_REDUCED || st == ST_TURNED_REDUCED;
    if (st == ST_VIDEO)
    {
        if (const char* bad = videoFormatBad(src.fmt))
        {
            return fail(c, ACF_HIP_E_INVALID, w + bad);
        }
        if (!(src.scale >= 0) || !std::isfinite(src.scale))
        {
            return fail(c, ACF_HIP_E_INVALID, w + "scale must be 0 (no resize) or a positive finite number");
        }
        // (the one check of the context in here: the open of another format refuses sub-batch streams before the geometry, every
        // other open after it and after the size against the plan — streamOpenYuv)
        if (open && !videoFormatIsDefault(src.fmt) && !c->kids.empty())
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, w + "not available with option \"streams\" > 1");
        }
        sized = src.orient != 0 || src.scale != 0 || src.srcRows != 0 || src.srcCols != 0;
        wide = src.fmt.bits > 8 && (src.orient != 0 || src.scale != 0);
        src.resized = src.scale != 0;
    }
    const bool turnedBad = sized && orientedArgsBad(src.srcRows, src.srcCols, src.orient);
    // (the pyramid entries refuse the sample width before the orient range and the size, a stream's open after them)
    if (wide && !(open && turnedBad))
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, w + "more than 8 bits a sample: upright and unreduced frames only (orient 0, scale 0)");
    }
    if (turnedBad)
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(src.who) + ": orient must be 0 .. 7 (ACF_HIP_ORIENT_*), src_rows and src_cols >= 1");
    }
    return ACF_HIP_OK;
}

// What the plan must be for — the second layer, for a source that passed the first: the upright size of an unreduced source is the
// plan's (a source that states no size has the plan's); a reduced source needs the tap tables of its upright size, which are built
// against the plan (resizedTables).  The ONE place that holds a frame size against the plan (planIngest and streamOpenYuv call it).
static int sourceAgainstPlan(acf_hip_ctx* c, const FrameSource& src)
{
    int rows = src.srcRows, cols = src.srcCols; // (a turned frame: orient first, then resize)
    if (src.orient & 1)
    {
        std::swap(rows, cols);
    }
    if (src.resized)
    {
        return resizedTables(c, src.who, rows, cols, src.scale);
    }
    if ((rows || cols) && (c->plan.H != rows || c->plan.W != cols))
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(src.who) + ": the plan must be for the upright size (acf_hip_oriented_dims of the frame size and orientation)");
    }
    return ACF_HIP_OK;
}

// The wide load form of k_ingest_yuv_oriented for NV12 / NV21-like descriptions of any size: luma samples 1 apart, chroma one plane
// of byte pairs, all of it four-aligned with the pointer
static bool yuvIsAlignedPairs(const YuvDescSrc& s, int& vFirst)
{
    const uintptr_t at = reinterpret_cast<uintptr_t>(s.base);
    const int64_t c0 = std::min(s.u.off, s.v.off);
    vFirst = s.v.off < s.u.off;
    return s.subX == 1 && s.y.sp == 1 && s.u.sp == 2 && s.v.sp == 2 && std::max(s.u.off, s.v.off) == c0 + 1 && s.u.sr == s.v.sr && s.u.sn == s.v.sn &&
           (at + uintptr_t(s.y.off)) % 4 == 0 && s.y.sr % 4 == 0 && s.y.sn % 4 == 0 && (at + uintptr_t(c0)) % 4 == 0 && s.u.sr % 4 == 0 && s.u.sn % 4 == 0;
}

// The staged form of k_ingest_oriented_resized marches a 64 x 64 reduced tile in bands of reduced rows; the band for tables t: the tile
// split into the fewest equal bands (64, 32, 22, 16, 13, 11, 10, 8 rows) such that the footprint of every band of every tile (rz_span,
// the kernel's own arithmetic) fits OS_STAGE dwords at the kernel's pitch (stored columns | 1; quarter turns: the band's rows are the
// stored columns).  0: not even bands of OS_MIN_BAND rows fit (scales under 1 / 4): the generic form.
static int orientedResizedBand(const ResizeTables& t, bool swap)
{
    const auto span = [&](bool y, int d0, int d1) {
        int f, l;
        rz_span(t.mode, y ? t.isy : t.isx, y ? t.rows : t.cols, (y ? t.ylin : t.xlin).data(), (y ? t.yrun : t.xrun).data(), (y ? t.ytap : t.xtap).data(), y, d0, d1, f, l);
        return l - f + 1;
    };
    int fw = 1;
    for (int x0 = 0; x0 < t.dcols; x0 += IG_T)
    {
        fw = std::max(fw, span(false, x0, std::min(x0 + IG_T, t.dcols) - 1));
    }
    for (int nb = 1; nb <= IG_T / OS_MIN_BAND; nb++)
    {
        const int b = cdiv(IG_T, nb);
        int fh = 1;
        for (int y0 = 0; y0 < t.drows; y0 += IG_T)
        {
            const int ny = std::min(IG_T, t.drows - y0);
            for (int yb = 0; yb < ny; yb += b)
            {
                fh = std::max(fh, span(true, y0 + yb, y0 + std::min(yb + b, ny) - 1));
            }
        }
        if ((swap ? int64_t(fw) * (fh | 1) : int64_t(fh) * (fw | 1)) <= OS_STAGE)
        {
            return b;
        }
    }
    return 0;
}

// One call's ingest, decided once (planIngest); PyramidRun::ingest only reads it
struct IngestPlan
{
    // the preludes, in this order: cvtColor first, as the apps do, in front of their Resizer (convert -> resize -> ingest)
    bool toRgb = false;        // k_yuv420_to_rgb8: the caller's NV12 / NV21 frames -> tight RGB in c->d_yuvRgb
    YuvSrc toRgbSrc{};
    bool resize = false;       // k_resize_u8 (the apps' Resizer, acf.cpp:117-148): frames of rz.rows x rz.cols -> c->rz.d_out
    const uint8_t* resizeSrc = nullptr;
    int resizeCpp = 0, resizeStride = 0;
    // the ingest kernel
    bool convert = false;      // it writes the converted colour planes (c->d_color), else planar ones (c->d_stage)
    int nOut = 0;              // ... this many a frame
    const uint8_t* in = nullptr; // the 8-bit kinds: the packed frames it reads and their layout
    U8Geom g{};
    const void* kernel = nullptr;
    union Second               // the kernel's second argument (k_ingest_u8 has none)
    {
        ResizedSrc resized;
        YuvSrc yuv420;
        ImageArgs image;
        YuvDescSrc yuv;
        ImageOrientedSrc imageOriented;
        YuvOrientedSrc yuvOriented;
        OrientedResizedSrc orientedResized;
        Yuv16Src yuv16;
        ViewSrc view;
    } second{};
    const char* profName = nullptr;   // (static strings: prof keeps the pointer)
    const char* launchName = nullptr;

    // (a kernel goes in together with the argument of its own type)
    void set(IngestKernel k) { kernel = reinterpret_cast<const void*>(k); }
    void set(YuvIngestKernel k, const YuvSrc& s) { kernel = reinterpret_cast<const void*>(k); second.yuv420 = s; }
    void set(ImageKernel k, const ImageArgs& s) { kernel = reinterpret_cast<const void*>(k); second.image = s; }
    void set(YuvDescKernel k, const YuvDescSrc& s) { kernel = reinterpret_cast<const void*>(k); second.yuv = s; }
    void set(ResizedKernel k, const ResizedSrc& s) { kernel = reinterpret_cast<const void*>(k); second.resized = s; }
    void set(ImageOrientedKernel k, const ImageOrientedSrc& s) { kernel = reinterpret_cast<const void*>(k); second.imageOriented = s; }
    void set(YuvOrientedKernel k, const YuvOrientedSrc& s) { kernel = reinterpret_cast<const void*>(k); second.yuvOriented = s; }
    void set(OrientedResizedKernel k, const OrientedResizedSrc& s) { kernel = reinterpret_cast<const void*>(k); second.orientedResized = s; }
    void set(Yuv16Kernel k, const Yuv16Src& s) { kernel = reinterpret_cast<const void*>(k); second.yuv16 = s; }
    void set(ViewKernel k, const ViewSrc& s) { kernel = reinterpret_cast<const void*>(k); second.view = s; }
};

// A source that is both resized and oriented (r.r.im or r.r.yuv filled in; c->rzIn holds the tables of the upright size): the form of
// k_ingest_oriented_resized, by what was measured (profiles/oriented_resized_entry.md).  Staged for quarter turns where the footprint fits
// (orientedResizedBand): there the generic form's lanes each read another stored row (3.2 x / 5.2 x slower at scale 1 / 2 and 80 / 150).
// Generic for rot 0 / 2 — its lanes already run along the stored rows, in either direction, and the stage did not beat it (1.03 against
// 0.74 ms at 1 / 2, 1.74 against 1.70 ms at 80 / 150) —, for footprints that do not fit, and when forced.
static void planOrientedResized(acf_hip_ctx* c, int kind, int mode, bool vec, OrientedResizedSrc s, const FrameSource& src, IngestPlan& ip)
{
    static const char* const names[2][3] = { { "k_ingest_oriented_resized_image_generic", "k_ingest_oriented_resized_yuv_generic", "k_ingest_oriented_resized_yuv_generic" },
        { "k_ingest_oriented_resized_image", "k_ingest_oriented_resized_yuv", "k_ingest_oriented_resized_yuv" } };
    s.r.t = resizeTaps(c->rzIn);
    s.o = orientSrc(src.orient, src.srcRows, src.srcCols);
    int& band = c->rzIn.osBand[s.o.swap];
    if (band < 0)
    {
        band = orientedResizedBand(c->rzIn.t, s.o.swap != 0);
    }
    const bool staged = s.o.swap && band > 0 && !fallbackForced(FB_ORIENTED_RESIZED_GENERIC);
    s.band = band;
    s.vec = vec;
    ip.set(orientedResizedKernel(kind, mode, staged), s);
    ip.profName = names[staged][kind];
    ip.launchName = "k_ingest_oriented_resized";
}

// The reduced sources of both kinds (r.im or r.yuv filled in; kind: RS_*): the source against the plan, which leaves the tables of
// the upright size in c->rzIn, then the apps' Resizer on the addressed bytes in the ingest kernel itself — k_ingest_resized, or for a
// turned frame k_ingest_oriented_resized (vec: its wide load form holds)
static int planReduced(acf_hip_ctx* c, const FrameSource& src, int kind, int mode, bool vec, ResizedSrc r, IngestPlan& ip)
{
    if (int rc = sourceAgainstPlan(c, src))
    {
        return rc;
    }
    if (src.orient)
    {
        OrientedResizedSrc o{};
        o.r = r;
        planOrientedResized(c, kind, mode, vec, o, src, ip);
        return ACF_HIP_OK;
    }
    r.t = resizeTaps(c->rzIn);
    ip.set(resizedKernel(kind, mode), r);
    ip.profName = kind == RS_IMAGE ? "k_ingest_resized_image" : "k_ingest_resized_yuv";
    ip.launchName = "k_ingest_resized";
    return ACF_HIP_OK;
}

// 8-bit ingest (ACF.cpp:114-119,137; MatP.cpp:51-73), fused with the colour conversion when there is one
static int planU8(acf_hip_ctx* c, const FrameSource& src, int mode, IngestPlan& ip)
{
    const int H = c->plan.H, W = c->plan.W, d_in = c->plan.d_in;
    const std::string who = std::string(src.who) + ": ";
    if (d_in == 5)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "a plan for five input planes (image + M, O) takes float frames");
    }
    const bool rz = c->rz.on, yuv = pixIsYuv(src.pix), fused = yuv && !rz && !fallbackForced(FB_YUV_UNFUSED);
    int rows = rz ? c->rz.rows : H, cols = rz ? c->rz.cols : W; // the caller's frames
    U8Geom& g = ip.g;
    if (const char* bad = u8Geom(src.pix, rows, cols, src.rowStride, c->yuv.chromaOff, c->yuv.frameStride, g))
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(src.who) + (rz && !yuv ? " (the unreduced frame): " : ": ") + bad);
    }
    if (!u8PlanesOk(g, d_in))
    {
        return fail(c, ACF_HIP_E_INVALID, who + (yuv && !fused ? "the plan's input planes (d) must be 3 for NV12 / NV21"
                                                              : "the plan's input planes (d) must be 3 for colour layouts (NV12 / NV21 included) and 1 for GRAY"));
    }
    ip.in = static_cast<const uint8_t*>(src.base);
    // a prelude leaves tight frames of the same pixel layout
    const auto tight = [&](const uint8_t* at) {
        ip.in = at;
        g.stride = cols * g.cpp;
        g.frameStride = int64_t(g.stride) * rows;
    };
    if (yuv && !fused)
    {
        const size_t need = size_t(c->maxBatch) * rows * cols * 3;
        if (c->yuvRgbBytes < need)
        {
            HIPCHK(c, hipStreamSynchronize(c->stream)); // (a batch in flight may still read the smaller buffer)
            devRelease(c, c->d_yuvRgb);
            c->yuvRgbBytes = 0;
            if (int rc = devAlloc(c, &c->d_yuvRgb, need))
            {
                return rc;
            }
            c->yuvRgbBytes = need;
        }
        ip.toRgb = true;
        ip.toRgbSrc = yuvSrc(ip.in, src.pix, rows, cols, g);
        g = U8Geom{ 3, 0, 0, 1, 2, false, 0, 0 };
        tight(c->d_yuvRgb);
    }
    if (rz)
    {
        ip.resize = true;
        ip.resizeSrc = ip.in;
        ip.resizeCpp = g.cpp;
        ip.resizeStride = g.stride;
        rows = H;
        cols = W;
        tight(c->rz.d_out);
    }
    bool aligned = (reinterpret_cast<uintptr_t>(ip.in) % 4 == 0) && (g.stride % 4 == 0);
    if (fused)
    {
        aligned = aligned && g.chromaOff % 4 == 0 && g.frameStride % 4 == 0;
        ip.set(yuvIngestKernel(mode, aligned), yuvSrc(ip.in, src.pix, H, W, g));
    }
    else
    {
        ip.set(ingestKernel(mode, aligned));
    }
    ip.profName = ip.launchName = fused ? "k_ingest_yuv420" : "k_ingest_u8";
    return ACF_HIP_OK;
}

// The image kind: images of any strides and element type (ACF.cpp:135-141 for CV_32FC3 and CV_8UC3; MatP.cpp:51-73), upright
// (k_ingest_image) or turned — the same description and load forms at srcRows x srcCols, placed upright (k_ingest_image_oriented);
// reduced: planReduced
static int planImage(acf_hip_ctx* c, const FrameSource& src, int mode, IngestPlan& ip)
{
    const int d_in = c->plan.d_in;
    const std::string who = std::string(src.who) + ": ";
    if (const char* bad = imageDescBad(&src.img))
    {
        return fail(c, ACF_HIP_E_INVALID, who + bad);
    }
    if (d_in == 5)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "a plan for five input planes (image + M, O) takes planar float frames");
    }
    if (src.img.channels != d_in)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "channels must be the plan's input planes (d)");
    }
    ImageArgs s = imageArgs(src.base, src.img);
    if (src.resized)
    {
        if (src.img.dtype != ACF_HIP_T_U8)
        {
            return fail(c, ACF_HIP_E_UNSUPPORTED, who + "dtype must be ACF_HIP_T_U8 (cv::resize's CV_32F arithmetic is not restated)");
        }
        ResizedSrc r{};
        r.im = s;
        return planReduced(c, src, RS_IMAGE, mode, imageLoadForm(src.base, src.img) == IM_ROWVEC, r, ip);
    }
    if (c->rz.on)
    {
        return inputResizeRefused(c, src.who, "the resize takes packed 8-bit frames");
    }
    if (int rc = sourceAgainstPlan(c, src))
    {
        return rc;
    }
    s.form = imageLoadForm(src.base, src.img);
    if (src.orient)
    {
        const OrientSrc o = orientSrc(src.orient, src.srcRows, src.srcCols);
        ip.set(imageOrientedKernel(src.img.dtype, mode), ImageOrientedSrc{ s, o });
        ip.profName = s.form == IM_GENERIC ? "k_ingest_image_oriented_generic" : (o.swap ? "k_ingest_image_oriented_cols" : "k_ingest_image_oriented_rows");
        ip.launchName = "k_ingest_image_oriented";
        return ACF_HIP_OK;
    }
    ip.set(imageKernel(src.img.dtype, mode), s);
    ip.profName = ip.launchName = "k_ingest_image";
    return ACF_HIP_OK;
}

// The YUV kind, three planes described by offsets and byte strides: cvtColor's BT.601 integer conversion (restated, kernels_input.hip.h),
// then the 8-bit image entry (ACF.cpp:114-119,135-141; MatP.cpp:51-73), in one kernel.  A format other than the default (cf) runs the
// same 8-bit kernels with the constants as an argument, under the same profile names; more than 8 bits is k_ingest_yuv16 (upright
// and unreduced: sourceArgsBad).  The format itself was checked where the call or the stream's open stated it.
static int planYuv(acf_hip_ctx* c, const FrameSource& src, int mode, IngestPlan& ip)
{
    const std::string who = std::string(src.who) + ": ";
    if (const char* bad = yuvDescBad(&src.yuv))
    {
        return fail(c, ACF_HIP_E_INVALID, who + bad);
    }
    if (c->plan.d_in != 3)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "the plan's input planes (d) must be 3");
    }
    const bool cf = !videoFormatIsDefault(src.fmt);
    const uint8_t* base = static_cast<const uint8_t*>(src.base);
    if (src.fmt.bits > 8)
    {
        if (const char* bad = video16DescBad(base, src.yuv))
        {
            return fail(c, ACF_HIP_E_INVALID, who + bad);
        }
        if (c->rz.on)
        {
            return inputResizeRefused(c, src.who, "the resize takes the 8-bit entries' frames");
        }
        if (int rc = sourceAgainstPlan(c, src))
        {
            return rc;
        }
        static const char* const names16[3] = { "k_ingest_yuv16_generic", "k_ingest_yuv16_planar", "k_ingest_yuv16_pairs" };
        Yuv16Src y{};
        y.yuv = yuvDescSrc(base, src.yuv);
        y.yuv.k = yuvCoef(src.fmt);
        y.shift = src.fmt.shift;
        y.mask = (1 << src.fmt.bits) - 1;
        const int form = yuv16LoadForm(y.yuv, y.vFirst);
        ip.set(yuv16Kernel(form, mode), y);
        ip.profName = names16[form];
        ip.launchName = "k_ingest_yuv16";
        return ACF_HIP_OK;
    }
    YuvDescSrc s = yuvDescSrc(base, src.yuv);
    if (cf)
    {
        s.k = yuvCoef(src.fmt);
    }
    if (src.resized)
    {
        const bool vec = src.orient && yuvLoadForm(s) == YD_PLANAR; // (the turned form's; yuvLoadForm leaves its findings in s)
        ResizedSrc r{};
        r.yuv = s;
        return planReduced(c, src, cf ? RS_YUV_CF : RS_YUV, mode, vec, r, ip);
    }
    if (c->rz.on)
    {
        return inputResizeRefused(c, src.who, "the resize takes the 8-bit entries' frames");
    }
    if (int rc = sourceAgainstPlan(c, src))
    {
        return rc;
    }
    if (src.orient)
    {
        // a turned frame: the description at srcRows x srcCols, the chroma sample chosen there, placed upright (k_ingest_yuv_oriented)
        YuvOrientedSrc y{};
        y.o = orientSrc(src.orient, src.srcRows, src.srcCols);
        y.form = yuvLoadForm(s);
        if (y.form == YD_GENERIC && yuvIsAlignedPairs(s, y.vFirst))
        {
            y.form = YO_SEMI;
        }
        y.yuv = s;
        ip.set(yuvOrientedKernel(mode, cf), y);
        ip.profName = y.form == YD_GENERIC ? "k_ingest_yuv_oriented_generic" : (y.o.swap ? "k_ingest_yuv_oriented_cols" : "k_ingest_yuv_oriented_rows");
        ip.launchName = "k_ingest_yuv_oriented";
        return ACF_HIP_OK;
    }
    YuvSrc semi;
    if (yuvIsSemiPlanar(base, src.yuv, c->plan.H, c->plan.W, semi))
    {
        const bool aligned = reinterpret_cast<uintptr_t>(semi.in) % 4 == 0 && semi.rowStride % 4 == 0 && semi.chromaOff % 4 == 0 && semi.in_fs % 4 == 0;
        semi.k = s.k;
        ip.set(yuvIngestKernel(mode, aligned, cf), semi); // (even sizes: never IG_LUV)
        ip.profName = ip.launchName = "k_ingest_yuv420";
        return ACF_HIP_OK;
    }
    static const char* const names[3] = { "k_ingest_yuv_generic", "k_ingest_yuv_planar", "k_ingest_yuv_packed422" };
    const int form = yuvLoadForm(s);
    ip.set(yuvDescKernel(form, mode, cf), s);
    ip.profName = names[form];
    ip.launchName = "k_ingest_yuv";
    return ACF_HIP_OK;
}

// The view kind (the header's "affine views of the stored frame"): frame i of the batch is the view views[i] of stored frame
// viewFrames[i], sampled from the frames as the description (image or YUV + format) and the orientation code state them, in
// k_ingest_view.  The checks are those of the oriented image / video entries about the description, and cut_crops' source's; the
// stored size is free of the plan's (the view maps one into the other).
static int planView(acf_hip_ctx* c, const FrameSource& src, int mode, IngestPlan& ip)
{
    const std::string who = std::string(src.who) + ": ";
    if (c->plan.d_in == 5)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "a plan for five input planes (image + M, O) takes planar float frames");
    }
    if (c->rz.on)
    {
        return inputResizeRefused(c, src.who, "a view scales by itself");
    }
    ViewSrc v{};
    int kind;
    if (!src.viewYuv)
    {
        if (src.img.channels != c->plan.d_in)
        {
            return fail(c, ACF_HIP_E_INVALID, who + "channels must be the plan's input planes (d)");
        }
        v.S.im = imageArgs(src.base, src.img);
        kind = src.img.dtype; // CUT_IMG_* = ACF_HIP_T_*
        v.C = src.img.channels;
        v.unit = src.img.dtype == ACF_HIP_T_U8 ? float(1.0 / 255.0) : 1.f;
    }
    else
    {
        if (c->plan.d_in != 3)
        {
            return fail(c, ACF_HIP_E_INVALID, who + "the plan's input planes (d) must be 3");
        }
        Yuv16Src& y = v.S.yuv;
        y.yuv = yuvDescSrc(static_cast<const uint8_t*>(src.base), src.yuv);
        y.yuv.k = yuvCoef(src.fmt);
        y.shift = src.fmt.shift;
        y.mask = (1 << src.fmt.bits) - 1;
        kind = src.fmt.bits > 8 ? CUT_YUV16 : (videoFormatIsDefault(src.fmt) ? CUT_YUV8 : CUT_YUV8_CF);
        v.C = 3;
        v.unit = src.fmt.bits == 8 ? float(1.0 / 255.0) : y.yuv.k.sc;
    }
    v.views = src.views;
    v.frames = src.viewFrames;
    v.nFrames = src.nStored;
    v.o = orientSrc(src.orient, src.srcRows, src.srcCols);
    v.Hu = v.o.swap ? src.srcCols : src.srcRows;
    v.Wu = v.o.swap ? src.srcRows : src.srcCols;
    v.s = src.samples;
    ip.set(viewKernel(kind, mode), v);
    ip.profName = src.viewYuv ? "k_ingest_view_yuv" : "k_ingest_view_image";
    ip.launchName = "k_ingest_view";
    return ACF_HIP_OK;
}

// The ingest of one call: the source held against the plan and the context's settings (what is refused, in the order the entries
// have always checked), then the kernel form, its arguments and its names.  The ONE place that decides them.
static int planIngest(acf_hip_ctx* c, const FrameSource& src, IngestPlan& ip)
{
    ip = IngestPlan{};
    // to the converted colour planes where the model converts (every colour space but hsv), else to planar planes in d_stage (hsv:
    // k_rgb2hsv follows like on a float frame; orig / isLuv: the pyramid reads them as they are)
    ip.convert = c->d_color && c->p.colorSpace != ACF_HIP_CS_HSV;
    const int mode = ingestMode(c, ip.convert);
    ip.nOut = (ip.convert && mode == IG_PLANAR) ? 3 : c->plan.d_in; // ORIG / RGB with a 1-plane input: replicate (chnsPyramid.cpp:242-243)
    return src.kind == SRC_U8      ? planU8(c, src, mode, ip)
           : src.kind == SRC_IMAGE ? planImage(c, src, mode, ip)
           : src.kind == SRC_VIEW  ? planView(c, src, mode, ip)
                                   : planYuv(c, src, mode, ip);
}

// the pyramid of a source, then the cascade on it: the run_ entries of every kind but planar float frames, and the stream
static int runSource(acf_hip_ctx* c, const FrameSource& src, int nF)
{
    const int rc = pyramidImpl(c, src, nF);
    return rc ? rc : acf_hip_detect(c);
}

// The two general entries, image and YUV: every exported entry of their kinds is one call of them that fills in what it states (st)
// and leaves the rest 0 — srcRows == srcCols == 0: the plan's size, orient 0: upright, scale 0: no resize, no format: the default.
// The pyramid alone, or the whole run (detect).  The order of the refusals is the entries' own: what the call states (sourceArgsBad),
// the pointers, then pyramidBody's (streams, plan, n_frames) and planIngest's.
static int imageEntry(acf_hip_ctx* c, bool detect, const char* who, const void* frames, int nF, const acf_hip_image_desc* desc, Stated st, int srcRows, int srcCols,
    int orient, double scale)
{
    if (int rc = needCtx(c)) return rc;
    FrameSource src{ SRC_IMAGE, frames, who, 0, 0, {}, {}, false, srcRows, srcCols, scale, orient };
    if (int rc = sourceArgsBad(c, who, st, src)) return rc;
    if (!frames || !desc)
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(who) + ": null frames or description");
    }
    src.img = *desc;
    return detect ? runSource(c, src, nF) : pyramidImpl(c, src, nF);
}
static int yuvEntry(acf_hip_ctx* c, bool detect, const char* who, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, Stated st, int srcRows, int srcCols,
    int orient, double scale, const acf_hip_yuv_format* fmt = nullptr)
{
    if (int rc = needCtx(c)) return rc;
    FrameSource src{ SRC_YUV, base, who, 0, 0, {}, {}, false, srcRows, srcCols, scale, orient, fmt ? *fmt : kDefaultVideoFormat };
    // (acf_hip_run_video alone among the run_ entries names itself, and only where its format, scale and sample width are refused;
    // everywhere else it says pyramid_video, as every run_ entry says its pyramid_ twin's name)
    if (int rc = sourceArgsBad(c, st == ST_VIDEO && detect ? "run_video" : who, st, src)) return rc;
    if (!base || !desc)
    {
        return fail(c, ACF_HIP_E_INVALID, std::string(who) + ": null base or description");
    }
    src.yuv = *desc;
    return detect ? runSource(c, src, nF) : pyramidImpl(c, src, nF);
}

// The general view entry: what the call states about its source (cut_crops' checks of an acf_hip_crop_source), its views and its
// samples, whatever the context; then pyramidBody's (streams, plan, n_views) and planView's.  A view call always runs plainly.
static int viewEntry(acf_hip_ctx* c, bool detect, const acf_hip_crop_source* s, const float* views, const int32_t* frames, int nViews, int samples)
{
    if (int rc = needCtx(c)) return rc;
    const char* const name = "pyramid_view";
    const std::string who = "pyramid_view: ";
    if (!s || !views || !s->base_dev)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null source, base or views");
    }
    if ((s->image != nullptr) == (s->yuv != nullptr))
    {
        return fail(c, ACF_HIP_E_INVALID, who + "exactly one of image and yuv describes the frames");
    }
    if (samples < 1 || samples > 4)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "samples must be 1 .. 4");
    }
    if (s->n_frames < 1 || orientedArgsBad(s->src_rows, s->src_cols, s->orient))
    {
        return fail(c, ACF_HIP_E_INVALID, who + "orient must be 0 .. 7 (ACF_HIP_ORIENT_*), n_frames, src_rows and src_cols >= 1");
    }
    FrameSource src{ SRC_VIEW, s->base_dev, name };
    src.srcRows = s->src_rows;
    src.srcCols = s->src_cols;
    src.orient = s->orient;
    src.views = views;
    src.viewFrames = frames;
    src.nStored = s->n_frames;
    src.samples = samples;
    if (s->image)
    {
        if (const char* bad = imageDescBad(s->image))
        {
            return fail(c, ACF_HIP_E_INVALID, who + bad);
        }
        if (reinterpret_cast<uintptr_t>(s->base_dev) % imageElemBytes(s->image->dtype))
        {
            return fail(c, ACF_HIP_E_INVALID, who + "base_dev must be a multiple of the element size");
        }
        src.img = *s->image;
    }
    else
    {
        src.viewYuv = true;
        src.fmt = s->fmt ? *s->fmt : kDefaultVideoFormat;
        if (const char* bad = videoFormatBad(src.fmt))
        {
            return fail(c, ACF_HIP_E_INVALID, who + bad);
        }
        if (const char* bad = yuvDescBad(s->yuv))
        {
            return fail(c, ACF_HIP_E_INVALID, who + bad);
        }
        if (src.fmt.bits > 8)
        {
            if (const char* bad = video16DescBad(s->base_dev, *s->yuv))
            {
                return fail(c, ACF_HIP_E_INVALID, who + bad);
            }
        }
        src.yuv = *s->yuv;
    }
    if (!frames && nViews > s->n_frames)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "without frame indices view i reads stored frame i: n_views must not exceed n_frames");
    }
    return detect ? runSource(c, src, nViews) : pyramidImpl(c, src, nViews);
}
} // namespace

int acf_hip_pyramid_view(acf_hip_ctx* c, const acf_hip_crop_source* src, const float* views, const int32_t* frames, int nViews, int samples)
{
    return viewEntry(c, false, src, views, frames, nViews, samples);
}

int acf_hip_run_view(acf_hip_ctx* c, const acf_hip_crop_source* src, const float* views, const int32_t* frames, int nViews, int samples)
{
    return viewEntry(c, true, src, views, frames, nViews, samples);
}

// ---- the views' host arithmetic: in double from the float inputs, results rounded to float
int acf_hip_view_from_box(const float box[4], double angle, int h, int w, float m[6])
{
    if (!box || !m || h < 1 || w < 1)
    {
        return ACF_HIP_E_INVALID;
    }
    const double bx = box[0], by = box[1], bw = box[2], bh = box[3];
    const double sx = bw / w, sy = bh / h, ca = std::cos(angle), sa = std::sin(angle);
    const double m0 = sx * ca, m1 = -sy * sa, m3 = sx * sa, m4 = sy * ca;
    const double cx = bx + bw / 2, cy = by + bh / 2;
    const double out[6] = { m0, m1, cx - (m0 * w + m1 * h) / 2, m3, m4, cy - (m3 * w + m4 * h) / 2 };
    for (int k = 0; k < 6; k++)
    {
        m[k] = float(out[k]);
    }
    return ACF_HIP_OK;
}

int acf_hip_view_quad(const float m[6], const int32_t det[4], float quad[8])
{
    if (!m || !det || !quad)
    {
        return ACF_HIP_E_INVALID;
    }
    float q[8];
    view_quad_of(m, det[0], det[1], det[2], det[3], q); // (kernels_merge.hip.h: the arithmetic k_merge_views shares)
    std::copy(q, q + 8, quad);
    return ACF_HIP_OK;
}

int acf_hip_view_box(const float m[6], const int32_t det[4], float box[4])
{
    if (!m || !det || !box)
    {
        return ACF_HIP_E_INVALID;
    }
    float o[4];
    view_box_of(m, det[0], det[1], det[2], det[3], o);
    std::copy(o, o + 4, box);
    return ACF_HIP_OK;
}

int acf_hip_view_form(const float m[6], int samples, int tileX, int tileY, int h, int w, int Hu, int Wu, int channels, int sampleBytes, int* form)
{
    if (!m || !form || samples < 1 || samples > 4 || h < 1 || w < 1 || Hu < 1 || Wu < 1 || (channels != 1 && channels != 3) ||
        (sampleBytes != 1 && sampleBytes != 2 && sampleBytes != 4) || tileX < 0 || tileY < 0 || tileX >= cdiv(w, IG_T) || tileY >= cdiv(h, IG_T))
    {
        return ACF_HIP_E_INVALID;
    }
    const ViewGrid g = view_grid(m, samples, Hu, Wu);
    const int x0 = tileX * IG_T, y0 = tileY * IG_T, nx = std::min(IG_T, w - x0), ny = std::min(IG_T, h - y0);
    *form = view_form(g, view_rect(g, x0, y0, nx, ny), nx, ny, channels, sampleBytes);
    return ACF_HIP_OK;
}

int acf_hip_pyramid_u8(acf_hip_ctx* c, const uint8_t* frames, int nF, int pix, int rowStride)
{
    if (int rc = needCtx(c)) return rc;
    return pyramidImpl(c, FrameSource{ SRC_U8, frames, "pyramid_u8", pix, rowStride }, nF);
}

int acf_hip_run_u8(acf_hip_ctx* c, const uint8_t* frames, int nF, int pix, int rowStride)
{
    if (int rc = needCtx(c)) return rc;
    return runSource(c, FrameSource{ SRC_U8, frames, "pyramid_u8", pix, rowStride }, nF);
}

int acf_hip_pyramid_image(acf_hip_ctx* c, const void* frames, int nF, const acf_hip_image_desc* desc)
{
    return imageEntry(c, false, "pyramid_image", frames, nF, desc, ST_PLAN, 0, 0, 0, 0);
}

int acf_hip_run_image(acf_hip_ctx* c, const void* frames, int nF, const acf_hip_image_desc* desc)
{
    return imageEntry(c, true, "pyramid_image", frames, nF, desc, ST_PLAN, 0, 0, 0, 0);
}

int acf_hip_pyramid_image_resized(acf_hip_ctx* c, const void* frames, int nF, const acf_hip_image_desc* desc, int srcRows, int srcCols, double scale)
{
    return imageEntry(c, false, "pyramid_image_resized", frames, nF, desc, ST_REDUCED, srcRows, srcCols, 0, scale);
}

int acf_hip_run_image_resized(acf_hip_ctx* c, const void* frames, int nF, const acf_hip_image_desc* desc, int srcRows, int srcCols, double scale)
{
    return imageEntry(c, true, "pyramid_image_resized", frames, nF, desc, ST_REDUCED, srcRows, srcCols, 0, scale);
}

int acf_hip_pyramid_image_oriented(acf_hip_ctx* c, const void* frames, int nF, const acf_hip_image_desc* desc, int srcRows, int srcCols, int orient)
{
    return imageEntry(c, false, "pyramid_image_oriented", frames, nF, desc, ST_TURNED, srcRows, srcCols, orient, 0);
}

int acf_hip_run_image_oriented(acf_hip_ctx* c, const void* frames, int nF, const acf_hip_image_desc* desc, int srcRows, int srcCols, int orient)
{
    return imageEntry(c, true, "pyramid_image_oriented", frames, nF, desc, ST_TURNED, srcRows, srcCols, orient, 0);
}

int acf_hip_pyramid_image_oriented_resized(acf_hip_ctx* c, const void* frames, int nF, const acf_hip_image_desc* desc, int srcRows, int srcCols, int orient, double scale)
{
    return imageEntry(c, false, "pyramid_image_oriented_resized", frames, nF, desc, ST_TURNED_REDUCED, srcRows, srcCols, orient, scale);
}

int acf_hip_run_image_oriented_resized(acf_hip_ctx* c, const void* frames, int nF, const acf_hip_image_desc* desc, int srcRows, int srcCols, int orient, double scale)
{
    return imageEntry(c, true, "pyramid_image_oriented_resized", frames, nF, desc, ST_TURNED_REDUCED, srcRows, srcCols, orient, scale);
}

int acf_hip_pyramid_yuv(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc)
{
    return yuvEntry(c, false, "pyramid_yuv", base, nF, desc, ST_PLAN, 0, 0, 0, 0);
}

int acf_hip_run_yuv(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc)
{
    return yuvEntry(c, true, "pyramid_yuv", base, nF, desc, ST_PLAN, 0, 0, 0, 0);
}

int acf_hip_pyramid_yuv_resized(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, int srcRows, int srcCols, double scale)
{
    return yuvEntry(c, false, "pyramid_yuv_resized", base, nF, desc, ST_REDUCED, srcRows, srcCols, 0, scale);
}

int acf_hip_run_yuv_resized(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, int srcRows, int srcCols, double scale)
{
    return yuvEntry(c, true, "pyramid_yuv_resized", base, nF, desc, ST_REDUCED, srcRows, srcCols, 0, scale);
}

int acf_hip_pyramid_yuv_oriented(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, int srcRows, int srcCols, int orient)
{
    return yuvEntry(c, false, "pyramid_yuv_oriented", base, nF, desc, ST_TURNED, srcRows, srcCols, orient, 0);
}

int acf_hip_run_yuv_oriented(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, int srcRows, int srcCols, int orient)
{
    return yuvEntry(c, true, "pyramid_yuv_oriented", base, nF, desc, ST_TURNED, srcRows, srcCols, orient, 0);
}

int acf_hip_pyramid_yuv_oriented_resized(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, int srcRows, int srcCols, int orient, double scale)
{
    return yuvEntry(c, false, "pyramid_yuv_oriented_resized", base, nF, desc, ST_TURNED_REDUCED, srcRows, srcCols, orient, scale);
}

int acf_hip_run_yuv_oriented_resized(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, int srcRows, int srcCols, int orient, double scale)
{
    return yuvEntry(c, true, "pyramid_yuv_oriented_resized", base, nF, desc, ST_TURNED_REDUCED, srcRows, srcCols, orient, scale);
}

int acf_hip_pyramid_video(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, const acf_hip_yuv_format* fmt, int srcRows, int srcCols, int orient,
    double scale)
{
    return yuvEntry(c, false, "pyramid_video", base, nF, desc, ST_VIDEO, srcRows, srcCols, orient, scale, fmt);
}

int acf_hip_run_video(acf_hip_ctx* c, const uint8_t* base, int nF, const acf_hip_yuv_desc* desc, const acf_hip_yuv_format* fmt, int srcRows, int srcCols, int orient,
    double scale)
{
    return yuvEntry(c, true, "pyramid_video", base, nF, desc, ST_VIDEO, srcRows, srcCols, orient, scale, fmt);
}

int acf_hip_oriented_resized_dims(int srcRows, int srcCols, int orient, double scale, int* h, int* w)
{
    int uh, uw;
    if (!h || !w || !std::isfinite(scale) || acf_hip_oriented_dims(srcRows, srcCols, orient, &uh, &uw))
    {
        return ACF_HIP_E_INVALID;
    }
    return acf_hip_resize_dims(uh, uw, scale, h, w);
}

int acf_hip_oriented_dims(int srcRows, int srcCols, int orient, int* h, int* w)
{
    if (!h || !w || orientedArgsBad(srcRows, srcCols, orient))
    {
        return ACF_HIP_E_INVALID;
    }
    *h = (orient & 1) ? srcCols : srcRows;
    *w = (orient & 1) ? srcRows : srcCols;
    return ACF_HIP_OK;
}

int acf_hip_unorient_rect(int orient, int srcRows, int srcCols, const int32_t in[4], int32_t out[4])
{
    if (!in || !out || orientedArgsBad(srcRows, srcCols, orient))
    {
        return ACF_HIP_E_INVALID;
    }
    // upright columns [x, x + w) and rows [y, y + h): the source index an upright index follows runs with it or against it
    const OrientSrc o = orientSrc(orient, srcRows, srcCols);
    const int32_t x = in[0], y = in[1], w = in[2], h = in[3];
    const int32_t r0 = o.swap ? x : y, nr = o.swap ? w : h; // along the source rows
    const int32_t c0 = o.swap ? y : x, nc = o.swap ? h : w; // along the source columns
    out[0] = o.revC ? srcCols - c0 - nc : c0;
    out[1] = o.revR ? srcRows - r0 - nr : r0;
    out[2] = nc;
    out[3] = nr;
    return ACF_HIP_OK;
}

int acf_hip_image_extent(const acf_hip_image_desc* d, int h, int w, int nF, int64_t* first, int64_t* last)
{
    if (!first || !last || imageDescBad(d) || h < 1 || w < 1 || nF < 1)
    {
        return ACF_HIP_E_INVALID;
    }
    int64_t lo = 0, hi = 0;
    const int64_t span[4] = { (nF - 1) * d->stride_n, (d->channels - 1) * d->stride_c, (h - 1) * d->stride_y, (w - 1) * d->stride_x };
    for (int64_t v : span)
    {
        (v < 0 ? lo : hi) += v;
    }
    *first = lo;
    *last = hi;
    return ACF_HIP_OK;
}

int acf_hip_yuv_extent(const acf_hip_yuv_desc* d, int h, int w, int nF, int64_t* first, int64_t* last)
{
    if (!first || !last || yuvDescBad(d) || h < 1 || w < 1 || nF < 1)
    {
        return ACF_HIP_E_INVALID;
    }
    yuvExtent(*d, h, w, nF, first, last);
    return ACF_HIP_OK;
}

int acf_hip_yuv_layout(int layout, int h, int w, int rowStride, acf_hip_yuv_desc* out, int64_t* frameBytes)
{
    if (!out || !frameBytes || h < 1 || w < 1 || rowStride < 0 || layout < ACF_HIP_YUV_NV12 || layout > ACF_HIP_YUV_YVYU)
    {
        return ACF_HIP_E_INVALID;
    }
    const bool packed = layout >= ACF_HIP_YUV_YUYV, semi = layout <= ACF_HIP_YUV_NV21;
    const int subX = layout == ACF_HIP_YUV_I444 ? 0 : 1, subY = (semi || layout == ACF_HIP_YUV_I420 || layout == ACF_HIP_YUV_YV12) ? 1 : 0;
    const int64_t rowBytes = packed ? 2 * int64_t(w) : w;
    const int64_t stride = rowStride > 0 ? rowStride : rowBytes;
    if (stride < rowBytes || (subX && w % 2) || (subY && h % 2) || (!packed && !semi && stride % 2))
    {
        return ACF_HIP_E_INVALID;
    }
    acf_hip_yuv_desc d{};
    d.sub_x = subX;
    d.sub_y = subY;
    int64_t fb;
    if (packed)
    {
        // macropixels of four bytes: Y0 U Y1 V / U Y0 V Y1 / Y0 V Y1 U
        const int yp = layout == ACF_HIP_YUV_UYVY ? 1 : 0, up = layout == ACF_HIP_YUV_YUYV ? 1 : (layout == ACF_HIP_YUV_UYVY ? 0 : 3),
                  vp = layout == ACF_HIP_YUV_YUYV ? 3 : (layout == ACF_HIP_YUV_UYVY ? 2 : 1);
        fb = stride * h;
        d.y = acf_hip_yuv_plane{ yp, fb, stride, 2 };
        d.u = acf_hip_yuv_plane{ up, fb, stride, 4 };
        d.v = acf_hip_yuv_plane{ vp, fb, stride, 4 };
    }
    else if (semi)
    {
        const int64_t chroma = stride * h; // the tight rule of the 8-bit entry (u8Geom)
        fb = chroma + stride * (h / 2);
        const int vFirst = layout == ACF_HIP_YUV_NV21;
        d.y = acf_hip_yuv_plane{ 0, fb, stride, 1 };
        d.u = acf_hip_yuv_plane{ chroma + vFirst, fb, stride, 2 };
        d.v = acf_hip_yuv_plane{ chroma + 1 - vFirst, fb, stride, 2 };
    }
    else
    {
        const int64_t cs = stride >> subX, plane = cs * (h >> subY), first = stride * h;
        fb = first + 2 * plane;
        const bool vFirst = layout == ACF_HIP_YUV_YV12;
        d.y = acf_hip_yuv_plane{ 0, fb, stride, 1 };
        d.u = acf_hip_yuv_plane{ first + (vFirst ? plane : 0), fb, cs, 1 };
        d.v = acf_hip_yuv_plane{ first + (vFirst ? 0 : plane), fb, cs, 1 };
    }
    *out = d;
    *frameBytes = fb;
    return ACF_HIP_OK;
}

// ---- what else takes an acf_hip_yuv_format beside the descriptor (the header's "video formats" section) ----

// The conversion alone, of any format, under the name of the entry that was called
static int videoToRgb(acf_hip_ctx* c, const std::string& who, const uint8_t* base, int nF, int rows, int cols, const acf_hip_yuv_desc* desc, const acf_hip_yuv_format& fmt,
    void* dst)
{
    if (int rc = needCtx(c)) return rc;
    if (const char* bad = videoFormatBad(fmt))
    {
        return fail(c, ACF_HIP_E_INVALID, who + bad);
    }
    if (!base || !desc || !dst)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null base, description or destination");
    }
    if (const char* bad = yuvDescBad(desc))
    {
        return fail(c, ACF_HIP_E_INVALID, who + bad);
    }
    if (nF < 1 || nF > 65535 || rows < 1 || cols < 1)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "n_frames 1 .. 65535, rows and cols >= 1");
    }
    const dim3 grid(cdiv(cols, 64), cdiv(rows, 4), nF);
    if (fmt.bits == 8)
    {
        const bool cf = !videoFormatIsDefault(fmt);
        YuvDescSrc s = yuvDescSrc(base, *desc);
        if (cf)
        {
            s.k = yuvCoef(fmt);
        }
        HIPCHK(c, hipSetDevice(c->device));
        prof(c, c->stream, "k_yuv_to_rgb8");
        hipLaunchKernelGGL((!cf ? k_yuv_to_rgb8<false> : k_yuv_to_rgb8<true>), grid, dim3(256), 0, c->stream, s, rows, cols, static_cast<uint8_t*>(dst));
        LAUNCHCHK(c, "k_yuv_to_rgb8");
        return ACF_HIP_OK;
    }
    const char* bad = video16DescBad(base, *desc);
    if (bad || reinterpret_cast<uintptr_t>(dst) % 2)
    {
        return fail(c, ACF_HIP_E_INVALID, who + (bad ? bad : "16-bit samples need an even destination"));
    }
    Yuv16Src y{};
    y.yuv = yuvDescSrc(base, *desc);
    y.yuv.k = yuvCoef(fmt);
    y.shift = fmt.shift;
    y.mask = (1 << fmt.bits) - 1;
    HIPCHK(c, hipSetDevice(c->device));
    prof(c, c->stream, "k_video_to_rgb16");
    hipLaunchKernelGGL(k_video_to_rgb16, grid, dim3(256), 0, c->stream, y, rows, cols, static_cast<uint16_t*>(dst));
    LAUNCHCHK(c, "k_video_to_rgb16");
    return ACF_HIP_OK;
}

int acf_hip_yuv_to_rgb8(acf_hip_ctx* c, const uint8_t* base, int nF, int rows, int cols, const acf_hip_yuv_desc* desc, uint8_t* dst)
{
    return videoToRgb(c, "yuv_to_rgb8: ", base, nF, rows, cols, desc, kDefaultVideoFormat, dst);
}

int acf_hip_video_to_rgb(acf_hip_ctx* c, const uint8_t* base, int nF, int rows, int cols, const acf_hip_yuv_desc* desc, const acf_hip_yuv_format* fmt, void* dst)
{
    return videoToRgb(c, "video_to_rgb: ", base, nF, rows, cols, desc, fmt ? *fmt : kDefaultVideoFormat, dst);
}

int acf_hip_video_extent(const acf_hip_yuv_desc* d, const acf_hip_yuv_format* fmtIn, int h, int w, int nF, int64_t* first, int64_t* last)
{
    const acf_hip_yuv_format fmt = fmtIn ? *fmtIn : kDefaultVideoFormat;
    if (!first || !last || yuvDescBad(d) || videoFormatBad(fmt) || h < 1 || w < 1 || nF < 1 || (fmt.bits > 8 && video16DescBad(nullptr, *d)))
    {
        return ACF_HIP_E_INVALID;
    }
    yuvExtent(*d, h, w, nF, first, last);
    if (fmt.bits > 8)
    {
        for (int i = 0; i < 3; i++)
        {
            last[i] += 1; // the high byte of the last word
        }
    }
    return ACF_HIP_OK;
}

int acf_hip_video_layout(int layout, const acf_hip_yuv_format* fmtIn, int h, int w, int rowStride, acf_hip_yuv_desc* out, int64_t* frameBytes)
{
    const acf_hip_yuv_format fmt = fmtIn ? *fmtIn : kDefaultVideoFormat;
    if (videoFormatBad(fmt))
    {
        return ACF_HIP_E_INVALID;
    }
    if (fmt.bits == 8)
    {
        return acf_hip_yuv_layout(layout, h, w, rowStride, out, frameBytes);
    }
    // two bytes a sample: the layout of w 16-bit words is the 8-bit layout of a row stride counted in words, every byte quantity doubled
    if (!out || !frameBytes || rowStride < 0 || rowStride % 2)
    {
        return ACF_HIP_E_INVALID;
    }
    acf_hip_yuv_desc d{};
    int64_t fb = 0;
    if (int rc = acf_hip_yuv_layout(layout, h, w, rowStride / 2, &d, &fb)) return rc;
    for (acf_hip_yuv_plane* p : { &d.y, &d.u, &d.v })
    {
        p->offset *= 2;
        p->stride_n *= 2;
        p->stride_row *= 2;
        p->stride_px *= 2;
    }
    *out = d;
    *frameBytes = 2 * fb;
    return ACF_HIP_OK;
}

int acf_hip_yuv_coeffs(const acf_hip_yuv_format* fmtIn, int64_t* out)
{
    const acf_hip_yuv_format fmt = fmtIn ? *fmtIn : kDefaultVideoFormat;
    if (!out || videoFormatBad(fmt))
    {
        return ACF_HIP_E_INVALID;
    }
    const YuvCoef k = yuvCoef(fmt);
    const int64_t v[8] = { k.yoff, k.cmid, k.omax, k.cy, k.cvr, k.cvg, k.cug, k.cub };
    std::copy(v, v + 8, out);
    return ACF_HIP_OK;
}

int acf_hip_u8_frame_bytes(int pix, int rows, int cols, int rowStride, int64_t* out)
{
    U8Geom g;
    if (!out || u8Geom(pix, rows, cols, rowStride, 0, 0, g))
    {
        return ACF_HIP_E_INVALID;
    }
    *out = g.frameStride;
    return ACF_HIP_OK;
}

int acf_hip_set_yuv_layout(acf_hip_ctx* c, int64_t chromaOff, int64_t frameStride)
{
    if (int rc = needPlan(c, "set_yuv_layout")) return rc;
    if (!c->kids.empty() || !c->slots.empty())
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "set_yuv_layout: not with option \"streams\" > 1; before acf_hip_stream_open");
    }
    if (chromaOff < 0 || frameStride < 0)
    {
        return fail(c, ACF_HIP_E_INVALID, "set_yuv_layout: negative offset or stride");
    }
    dropGraph(c);
    c->yuv.chromaOff = chromaOff; // (held against the frames' row stride where that is known: the run / open call)
    c->yuv.frameStride = frameStride;
    return ACF_HIP_OK;
}

int acf_hip_resize_dims(int rows, int cols, double scale, int* out_rows, int* out_cols)
{
    if (!out_rows || !out_cols || rows < 1 || cols < 1 || !(scale > 0))
    {
        return ACF_HIP_E_INVALID;
    }
    resizeDims(rows, cols, scale, *out_rows, *out_cols);
    return (*out_rows >= 1 && *out_cols >= 1) ? ACF_HIP_OK : ACF_HIP_E_INVALID;
}

int acf_hip_set_input_resize(acf_hip_ctx* c, int srcRows, int srcCols, double scale)
{
    if (int rc = needPlan(c, "set_input_resize", " (for the reduced size, acf_hip_resize_dims)")) return rc;
    if (!c->kids.empty() || !c->slots.empty())
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, "set_input_resize: not with option \"streams\" > 1; before acf_hip_stream_open");
    }
    dropGraph(c);
    if (srcRows <= 0 || srcCols <= 0)
    {
        c->rz.on = false;
        return ACF_HIP_OK;
    }
    if (c->rz.d_out && c->rz.rows == srcRows && c->rz.cols == srcCols && c->rz.scale == scale)
    {
        c->rz.on = true; // same geometry as the tables already on the device (a re-opened stream): nothing to build
        return ACF_HIP_OK;
    }
    return installResizeTables(c, "set_input_resize", c->rz, srcRows, srcCols, scale, true);
}
