// cut_run.hip.h — part of acf_hip.hip (included there and nowhere else): crops of the stored frame, the stage behind the detections
// (the header's "crops of the stored frame" section; kernel k_cut_crops, kernels_cut.hip.h).
//   cutChecked               what a call states about its source and its spec, checked on the host before any launch: the refusal, or the
//                            kernel's arguments without the crop list
//   launchCut                the one launch, under the profile name k_cut_crops
//   acf_hip_cut_crops        a caller's boxes; acf_hip_cut_detections: the records and counts of the context's last batch, read on the
//                            device in the same launch (d_nmsDets / d_nmsCounts or cs.d_dets / cs.d_counts, as k_export reads them)
//   acf_hip_crop_box / _crop_bytes / _crop_form   host arithmetic: cut_box, the crop's size, cut_form
// Nothing here allocates, waits for the device or touches what acf_hip_run left behind (a captured graph stays valid).
#pragma once

namespace
{

struct CutCall
{
    CutArgs a{};
    CutSource S{};
    int kind = 0;
};

const char* cutSpecBad(const acf_hip_crop_spec* s, bool dets)
{
    if (!s)
    {
        return "null spec";
    }
    if (s->out_h < 1 || s->out_h > 512 || s->out_w < 1 || s->out_w > 512)
    {
        return "out_h and out_w must be 1 .. 512";
    }
    if (s->samples < 1 || s->samples > 4)
    {
        return "samples must be 1 .. 4";
    }
    if (s->dtype < ACF_HIP_T_U8 || s->dtype > ACF_HIP_T_F32)
    {
        return "unknown dtype";
    }
    if (s->layout != 0 && s->layout != 1)
    {
        return "layout must be 0 (planar) or 1 (packed)";
    }
    if (s->reserved != 0)
    {
        return "reserved must be 0";
    }
    if (dets && (s->max_per_frame < 1 || s->max_per_frame > ACF_HIP_NMS_CAP))
    {
        return "max_per_frame must be 1 .. ACF_HIP_NMS_CAP";
    }
    if (dets && !(s->grow > 0.f && std::isfinite(s->grow)))
    {
        return "grow must be a positive finite number";
    }
    return nullptr;
}

// The source and the spec of a call -> the kernel's arguments (everything but the crop list), or the refusal
int cutChecked(acf_hip_ctx* c, const std::string& who, const acf_hip_crop_source* src, const acf_hip_crop_spec* spec, bool dets, void* dst, CutCall& out)
{
    if (!src || !dst || !src->base_dev)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null source, base or destination");
    }
    if (const char* bad = cutSpecBad(spec, dets))
    {
        return fail(c, ACF_HIP_E_INVALID, who + bad);
    }
    if ((src->image != nullptr) == (src->yuv != nullptr))
    {
        return fail(c, ACF_HIP_E_INVALID, who + "exactly one of image and yuv describes the frames");
    }
    if (src->n_frames < 1 || orientedArgsBad(src->src_rows, src->src_cols, src->orient))
    {
        return fail(c, ACF_HIP_E_INVALID, who + "orient must be 0 .. 7 (ACF_HIP_ORIENT_*), n_frames, src_rows and src_cols >= 1");
    }
    CutArgs& a = out.a;
    bool codes8 = true; // the source holds 8-bit codes
    if (src->image)
    {
        if (const char* bad = imageDescBad(src->image))
        {
            return fail(c, ACF_HIP_E_INVALID, who + bad);
        }
        if (reinterpret_cast<uintptr_t>(src->base_dev) % imageElemBytes(src->image->dtype))
        {
            return fail(c, ACF_HIP_E_INVALID, who + "base_dev must be a multiple of the element size");
        }
        out.S.im = imageArgs(src->base_dev, *src->image);
        out.kind = src->image->dtype; // CUT_IMG_* = ACF_HIP_T_*
        a.C = src->image->channels;
        codes8 = src->image->dtype == ACF_HIP_T_U8;
        a.unit = codes8 ? float(1.0 / 255.0) : 1.f;
    }
    else
    {
        const acf_hip_yuv_format fmt = src->fmt ? *src->fmt : kDefaultVideoFormat;
        if (const char* bad = videoFormatBad(fmt))
        {
            return fail(c, ACF_HIP_E_INVALID, who + bad);
        }
        if (const char* bad = yuvDescBad(src->yuv))
        {
            return fail(c, ACF_HIP_E_INVALID, who + bad);
        }
        if (fmt.bits > 8)
        {
            if (const char* bad = video16DescBad(src->base_dev, *src->yuv))
            {
                return fail(c, ACF_HIP_E_INVALID, who + bad);
            }
        }
        Yuv16Src& y = out.S.yuv;
        y.yuv = yuvDescSrc(static_cast<const uint8_t*>(src->base_dev), *src->yuv);
        y.yuv.k = yuvCoef(fmt);
        y.shift = fmt.shift;
        y.mask = (1 << fmt.bits) - 1;
        out.kind = fmt.bits > 8 ? CUT_YUV16 : (videoFormatIsDefault(fmt) ? CUT_YUV8 : CUT_YUV8_CF);
        a.C = 3;
        codes8 = fmt.bits == 8;
        a.unit = codes8 ? float(1.0 / 255.0) : y.yuv.k.sc;
    }
    if (spec->dtype == ACF_HIP_T_U8 && !codes8)
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, who + "uint8 crops come from 8-bit codes only (a uint8 image, 8-bit video)");
    }
    if (!c->kids.empty())
    {
        return fail(c, ACF_HIP_E_UNSUPPORTED, who + "not available with option \"streams\" > 1");
    }
    if (reinterpret_cast<uintptr_t>(dst) % imageElemBytes(spec->dtype))
    {
        return fail(c, ACF_HIP_E_INVALID, who + "dst_dev must be a multiple of the element size");
    }
    a.nFrames = src->n_frames;
    a.o = orientSrc(src->orient, src->src_rows, src->src_cols);
    a.Hu = a.o.swap ? src->src_cols : src->src_rows;
    a.Wu = a.o.swap ? src->src_rows : src->src_cols;
    a.oh = spec->out_h;
    a.ow = spec->out_w;
    a.s = spec->samples;
    a.dtype = spec->dtype;
    a.layout = spec->layout;
    a.dst = static_cast<uint8_t*>(dst);
    a.cropBytes = int64_t(a.oh) * a.ow * a.C * imageElemBytes(spec->dtype);
    return ACF_HIP_OK;
}

int launchCut(acf_hip_ctx* c, const CutCall& k, int64_t slots)
{
    using Kernel = void (*)(CutArgs, CutSource);
    static const Kernel kernels[] = { k_cut_crops<CUT_IMG_U8>, k_cut_crops<CUT_IMG_F16>, k_cut_crops<CUT_IMG_BF16>, k_cut_crops<CUT_IMG_F32>, k_cut_crops<CUT_YUV8>,
        k_cut_crops<CUT_YUV8_CF>, k_cut_crops<CUT_YUV16> };
    if (slots < 1)
    {
        return ACF_HIP_OK;
    }
    if (slots > 0x7fffffff)
    {
        return fail(c, ACF_HIP_E_INVALID, "cut: more than 2^31 - 1 crop slots");
    }
    HIPCHK(c, hipSetDevice(c->device));
    prof(c, c->stream, "k_cut_crops");
    hipLaunchKernelGGL(kernels[k.kind], dim3(unsigned(slots)), dim3(256), 0, c->stream, k.a, k.S);
    LAUNCHCHK(c, "k_cut_crops");
    prof(c, c->stream, "(end)");
    return ACF_HIP_OK;
}

} // namespace

int acf_hip_cut_crops(acf_hip_ctx* c, const acf_hip_crop_source* src, const float* boxes, const int32_t* frames, int n, const acf_hip_crop_spec* spec, void* dst)
{
    if (int rc = needCtx(c)) return rc;
    const std::string who = "cut_crops: ";
    CutCall k;
    if (int rc = cutChecked(c, who, src, spec, false, dst, k)) return rc;
    if (n < 0 || (n > 0 && (!boxes || !frames))) // (an empty list has no address)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null boxes or frame indices, or n < 0");
    }
    k.a.boxes = boxes;
    k.a.frames = frames;
    return launchCut(c, k, n);
}

int acf_hip_cut_detections(acf_hip_ctx* c, const acf_hip_crop_source* src, double detScale, const acf_hip_crop_spec* spec, void* dst, float* boxesOut,
    int32_t* countsOut)
{
    if (int rc = needCtx(c)) return rc;
    const std::string who = "cut_detections: ";
    CutCall k;
    if (int rc = cutChecked(c, who, src, spec, true, dst, k)) return rc;
    if (!countsOut)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "null counts_out_dev");
    }
    if (!(detScale >= 0) || !std::isfinite(detScale))
    {
        return fail(c, ACF_HIP_E_INVALID, who + "det_scale must be 0 (no resize) or a positive finite number");
    }
    if (!c->hasPlan || !c->detectValid)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "no detections (call acf_hip_detect or acf_hip_run* first)");
    }
    if (c->viewRun)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "the last run was a view (its boxes are in view coordinates: acf_hip_merge_views or acf_hip_view_box, then acf_hip_cut_crops)");
    }
    if (src->n_frames != c->lastBatch)
    {
        return fail(c, ACF_HIP_E_INVALID, who + "n_frames must be the last batch's");
    }
    int h = 0, w = 0;
    const int rc = detScale == 0 ? acf_hip_oriented_dims(src->src_rows, src->src_cols, src->orient, &h, &w)
                                 : acf_hip_oriented_resized_dims(src->src_rows, src->src_cols, src->orient, detScale, &h, &w);
    if (rc || h != c->plan.H || w != c->plan.W)
    {
        return fail(c, ACF_HIP_E_INVALID,
            who + "the plan must be for the frames' upright size reduced by det_scale (acf_hip_oriented_resized_dims; acf_hip_oriented_dims for det_scale 0)");
    }
    const bool nms = nmsActive(c);
    k.a.dets = nms ? c->d_nmsDets : c->cs.d_dets;
    k.a.counts = nms ? c->d_nmsCounts : c->cs.d_counts;
    k.a.maxHits = c->maxHits;
    k.a.K = spec->max_per_frame;
    k.a.inv = detScale == 0 ? 1.f : 1.f / float(detScale);
    k.a.grow = spec->grow;
    k.a.boxesOut = boxesOut;
    k.a.countsOut = countsOut;
    return launchCut(c, k, int64_t(c->lastBatch) * spec->max_per_frame);
}

int acf_hip_crop_box(const int32_t det[4], double detScale, float grow, float out[4])
{
    if (!det || !out)
    {
        return ACF_HIP_E_INVALID;
    }
    float o[4];
    cut_box(det[0], det[1], det[2], det[3], detScale == 0 ? 1.f : 1.f / float(detScale), grow, o);
    std::copy(o, o + 4, out);
    return ACF_HIP_OK;
}

int acf_hip_crop_bytes(const acf_hip_crop_spec* spec, int channels, int64_t* bytes)
{
    if (cutSpecBad(spec, false) || !bytes || (channels != 1 && channels != 3))
    {
        return ACF_HIP_E_INVALID;
    }
    *bytes = int64_t(spec->out_h) * spec->out_w * channels * imageElemBytes(spec->dtype);
    return ACF_HIP_OK;
}

int acf_hip_crop_form(const acf_hip_crop_spec* spec, const float box[4], int Hu, int Wu, int channels, int sampleBytes, int* form)
{
    if (cutSpecBad(spec, false) || !box || !form || Hu < 1 || Wu < 1 || (channels != 1 && channels != 3) || (sampleBytes != 1 && sampleBytes != 2 && sampleBytes != 4))
    {
        return ACF_HIP_E_INVALID;
    }
    *form = cut_form(spec->out_h, spec->out_w, spec->samples, box[0], box[1], box[2], box[3], Hu, Wu, channels, sampleBytes);
    return ACF_HIP_OK;
}
