// HipDetector.h — host-side C++ mirror of the reference's acf::Detector for the
// chnsPyramid + acfDetect hot path, backed by libacf_hip.so (MI355X / gfx950).
//
// Same method names, argument meaning and error behaviour as acf::Detector
// (reference src/lib/acf/acf/ACF.h:50-624, ObjectDetector.h:31-48); it plays
// the role acf::GLDetector plays for the GL backend (src/app/acf/GLDetector.h:
// 28-52): build the pyramid on the device, then run the multi-scale search.
// OpenCV is not available in this build image, so the three cv:: value types
// the API traffics in are restated here with the same member names; a
// maintainer wiring this into the reference replaces them by the cv:: ones
// (INTEGRATION.md shows the subclass).
//
// Layout contract (reference MatP.cpp:51-73, ACF.cpp:137): every plane is the
// TRANSPOSED image, float[rows = image width][cols = image height] with
// image-y contiguous.  cv::Size members for modelDs/modelDsPad/pad/minDs hold
// {width = image-height axis, height = image-width axis} (ACFIO.h:168-181);
// this class keeps that convention at its surface and converts to the C
// ABI's upright h/w names internally.
#pragma once

#include "acf_hip_loader.h"

#include <array>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <iosfwd>
#include <string>
#include <memory>
#include <vector>

namespace acf
{

struct Size
{
    int width = 0, height = 0;
    Size() = default;
    Size(int w, int h) : width(w), height(h) {}
    int area() const { return width * height; }
    bool operator==(const Size& o) const { return width == o.width && height == o.height; }
};

struct Size2d
{
    double width = 0, height = 0;
};

struct Rect
{
    int x = 0, y = 0, width = 0, height = 0;
    Rect() = default;
    Rect(int x_, int y_, int w_, int h_) : x(x_), y(y_), width(w_), height(h_) {}
    bool operator==(const Rect& o) const { return x == o.x && y == o.y && width == o.width && height == o.height; }
};

// Planar float image (reference MatP.h:25-190): `channels` planes of rows x cols,
// stored back to back (plane stride rows*cols), cols contiguous.
class MatP
{
public:
    MatP() = default;
    MatP(int rows, int cols, int channels) { create(rows, cols, channels); }
    // non-owning view over caller memory (the reference wraps cv::Mat headers the same way, MatP.cpp:51-73)
    MatP(int rows, int cols, int channels, float* data) : m_rows(rows), m_cols(cols), m_channels(channels), m_ptr(data) {}
    MatP(const MatP& o) { *this = o; }
    MatP& operator=(const MatP& o)
    {
        if (this != &o)
        {
            m_rows = o.m_rows;
            m_cols = o.m_cols;
            m_channels = o.m_channels;
            m_store = o.m_store;
            m_ptr = o.m_store.empty() ? o.m_ptr : m_store.data(); // owning copies re-point; views stay views
        }
        return *this;
    }
    void create(int rows, int cols, int channels)
    {
        m_rows = rows;
        m_cols = cols;
        m_channels = channels;
        m_store.assign(size_t(rows) * cols * channels, 0.f);
        m_ptr = m_store.data();
    }
    int rows() const { return m_rows; }
    int cols() const { return m_cols; }
    int channels() const { return m_channels; }
    bool empty() const { return !m_ptr || !m_rows || !m_cols || !m_channels; }
    Size size() const { return Size(m_cols, m_rows); }
    float* operator[](int c) { return m_ptr + size_t(c) * m_rows * m_cols; }
    const float* operator[](int c) const { return m_ptr + size_t(c) * m_rows * m_cols; }
    float* data() { return m_ptr; }
    const float* data() const { return m_ptr; }
    size_t numel() const { return size_t(m_rows) * m_cols * m_channels; }

private:
    int m_rows = 0, m_cols = 0, m_channels = 0;
    float* m_ptr = nullptr;
    std::vector<float> m_store;
};

// cv::Exception stand-in: precondition failures throw (reference: CV_Assert), the hot path returns 0.
class Exception : public std::runtime_error
{
public:
    Exception(int code_, const std::string& what) : std::runtime_error(what), code(code_) {}
    int code;
};

class HipDetector
{
public:
    using RealVec = std::vector<double>;
    using RectVec = std::vector<Rect>;

    // The fields of the Options tree (ACF.h:68-275) the hot path reads, flattened.
    struct Options
    {
        struct Nms
        {
            std::string type = "maxg"; // acfTrain default pNms; bbNms.cpp:229-304 handles max / maxg / none
            double thr = -1.7976931348623157e308;
            double overlap = 0.65;
            std::string ovrDnm = "min";
        } pNms;
        struct Pyramid
        {
            struct Chns
            {
                int shrink = 4;
                bool isLuv = false; // ACF.h:175: the input planes are LUV already (chnsPyramid.cpp:228 propagates Detector::setIsLuv)
                struct Color { int enabled = 1; double smooth = 1; std::string colorSpace = "luv"; } pColor;
                struct GradMag { int enabled = 1; int colorChn = 0; int normRad = 5; double normConst = 0.005; int full = 0; } pGradMag;
                struct GradHist { int enabled = 1; int binSize = 0; int nOrients = 6; int softBin = 0; } pGradHist;
            } pChns;
            int nPerOct = 8, nOctUp = 0, nApprox = 7;
            std::vector<double> lambdas{ 0.0, 0.1105, 0.1083 };
            Size pad{ 0, 0 };    // {width = image-height axis, height = image-width axis}
            Size minDs{ 16, 16 };
            double smooth = 1;
        } pPyramid;
        Size modelDs{ 16, 16 }, modelDsPad{ 16, 16 };
        // LDCF (toolbox opts.filters, BASELINE cfg 5; not in the reference's Options tree): k filters of 5x5 per channel applied to
        // every level before the cascade, which then runs at shrink*2.  Layout [k][nChns][5][5] = MATLAB memory order of fs(:,:,c,f).
        int ldcfK = 0;
        std::vector<float> ldcfFilters;
        int stride = 4;
        double cascThr = -1;
        double cascCal = 0;
    };

    // Detector::Classifier (ACF.h:292-310): row-major [nTrees][nTreeNodes] (after ACFIO.cpp:61-67's transpose).
    struct Classifier
    {
        int nTrees = 0, nTreeNodes = 0, treeDepth = 0;
        std::vector<uint32_t> fids, child;
        std::vector<float> thrs, hs;
        std::vector<uint8_t> thrsU8; // prescaled thresholds (x255) for uint8_t channels (ACF.h:305); filled on first use if empty
    };

    // Detector::Modify (ACF.h:391-408): the subset acfModify may override (acfModify.cpp:83-152).
    struct Modify
    {
        bool has_nPerOct = false, has_nOctUp = false, has_nApprox = false, has_lambdas = false, has_pad = false,
             has_minDs = false, has_stride = false, has_cascThr = false, has_cascCal = false;
        int nPerOct = 0, nOctUp = 0, nApprox = 0, stride = 0;
        std::vector<double> lambdas;
        Size pad, minDs;
        double cascThr = 0, cascCal = 0;
    };

    // Detector::Pyramid (ACF.h:364-389).  data[i][0] is level i's fused channel
    // buffer [nChns planes][wP rows][hP cols] (ACF.h:653-672 fuseChannels).
    struct Pyramid
    {
        int nTypes = 0, nScales = 0, nChns = 0;
        std::vector<std::vector<MatP>> data;
        std::vector<double> lambdas, scales;
        std::vector<Size2d> scaleshw;
        // ACF.h:377-378 ".rois - [LEVELS x CHANNELS] array for channel access": when rois[i] is not empty, data[i][0] is an
        // ATLAS plane (the GL backend's texture read-back, GPUACF.cpp) whose channels sit side by side: channel z starts
        // (rois[i][1].x - rois[i][0].x) * z elements after the plane's origin, element (c, r) of a channel c * rowStride + r
        // further (computeChannelIndex, acfDetect1.cpp:346-366, GPU_ACF_TRANSPOSE form); rois[i][z].{height, width} = the
        // channel's {columns c, rows r}.  The plane's cols() is its row stride.
        std::vector<std::vector<Rect>> rois;
        void clear()
        {
            rois.clear();
            data.clear();
            lambdas.clear();
            scales.clear();
            scaleshw.clear();
            nScales = 0;
        }
    };

    // Detector::Detection (ACF.h:510-525)
    struct Detection
    {
        Rect roi;
        double score = 0;
    };
    using DetectionVec = std::vector<Detection>;

    // Detector::Channels (ACF.h:326-340): what chnsCompute returns — one MatP per enabled channel type, in the order colour,
    // gradient magnitude, gradient histogram, each [type's channels][w / shrink rows][h / shrink cols]
    struct Channels
    {
        Options::Pyramid::Chns pChns;
        int nTypes = 0;
        std::vector<MatP> data;
        struct Info
        {
            std::string name;
            int nChns = 0;
            std::string padWith;
        };
        std::vector<Info> info;
    };

    // Detector::MatLoggerType (ACF.h:57): called with one plane and a tag "<name>:<cols>x<rows>"
    using MatLoggerType = std::function<int(const MatP&, const std::string&)>;
    // the reference's stream logger is a std::shared_ptr<spdlog::logger> (ACF.h:583-586; spdlog is not in this image): a text sink
    using StreamLoggerType = std::function<void(const std::string&)>;

    Options opts;
    Classifier clf;

    HipDetector() = default; // !good() until a model is supplied
    HipDetector(const Options& o, const Classifier& c, int device = 0);
    // Detector(filename) / Detector(istream, hint) (ACF.h:59-66): "*.cpb" = the reference's cereal files (ModelIO.h)
    explicit HipDetector(const std::string& filename, int device = 0);
    HipDetector(std::istream& is, const std::string& hint = {}, int device = 0);
    ~HipDetector();
    HipDetector(const HipDetector&) = delete;
    HipDetector& operator=(const HipDetector&) = delete;

    bool good() const { return m_good; }
    explicit operator bool() const { return m_good; }
    void setModel(const Options& o, const Classifier& c, int device = 0);

    // ObjectDetector knobs (ObjectDetector.h:37-47, ACF.h:495-595)
    void setDoNonMaximaSuppression(bool flag) { m_doNms = flag; }
    bool getDoNonMaximaSuppression() const { return m_doNms; }
    void setMaxDetectionCount(size_t n) { m_maxDetectionCount = n; }
    void setDetectionScorePruneRatio(double r) { m_detectionScorePruneRatio = r; }
    void setIsLuv(bool flag) { m_isLuv = flag; m_dirty = true; }
    bool getIsLuv() const { return m_isLuv; }
    void setIsTranspose(bool flag) { m_isTranspose = flag; }
    bool getIsTranspose() const { return m_isTranspose; }
    // Detector::setDoParallel (ACF.h:410: cv::parallel_for_ over scales): the real scales of a batch on streams of the context
    // beside each other (default, lowest latency) or all on one stream (several detectors side by side on one GPU)
    void setDoParallel(bool flag);
    // acf_hip_set_option (include/acf_hip.h): backend knobs without a counterpart among the reference's setters
    void setOption(const std::string& key, int value);
    void setIsRowMajor(bool flag) { m_isRowMajor = flag; } // ACF.h:588-595: stored for callers that orient the window size by it
    bool getIsRowMajor() const { return m_isRowMajor; }
    Size getWindowSize() const { return opts.modelDs; }
    // The apps' Resizer (src/app/acf/acf.cpp:117-148; GPUDetectionPipeline.cpp:250-266 computeDetectionWidth): search for objects of
    // at least `width` pixels — the packed 8-bit entries (operator()(packed ...), streamOpen / streamSubmit) reduce every frame by
    // scale = float(getWindowSize().width) / float(width) on the device (cv::resize: INTER_AREA when reducing, INTER_LINEAR else;
    // OpenCV's CV_8U arithmetic restated, parity unpinned: include/acf_hip.h) and map the boxes back with cv::Rect2f(o) * (1.f / scale).
    // width < 0 (default): off.
    void setMinObjectWidth(int width) { m_minObjectWidth = width; m_dirty = true; }
    int getMinObjectWidth() const { return m_minObjectWidth; }
    float inputScale() const { return m_minObjectWidth >= 0 ? float(getWindowSize().width) / float(m_minObjectWidth) : 1.f; }
    static Rect unscale(const Rect& o, float scale); // Resizer::operator()(objects) for one box
    // Rotated and mirrored frames (a decoder's rotation tag, a mirroring front camera): detectImages, detectYuv and streamOpenYuv take
    // the frames as they are stored, rows x cols, in orientation `orient` (ACF_HIP_ORIENT_*: rot + 4 * mirror; the upright frame is
    // the stored one mirrored left-right first, then turned rot quarter turns clockwise) and search the upright frame — the ingest
    // kernel reads the stored frame where it lies (include/acf_hip.h, acf_hip_run_image_oriented / acf_hip_run_yuv_oriented).  Boxes
    // come back in the UPRIGHT frame's coordinates; unorientRect maps one to the stored frame.  0 (default): off.  Together with
    // setMinObjectWidth the frame is turned upright first and then reduced, still in one kernel (acf_hip_run_image_oriented_resized /
    // acf_hip_run_yuv_oriented_resized); the boxes are unscaled as always, so they are in the upright FULL-SIZE frame.
    void setInputOrientation(int orient) { m_orient = orient; }
    int getInputOrientation() const { return m_orient; }

    // The sample width, matrix and range of the frames detectYuv and streamOpenYuv take (include/acf_hip.h, acf_hip_yuv_format: 8 bits
    // or 9 .. 16-bit little-endian words, BT.601 / BT.709 / BT.2020, limited or full range); the default {8, 0, BT601, 0} is cvtColor's
    // arithmetic.  Honoured together with setInputOrientation and setMinObjectWidth (acf_hip_run_video / acf_hip_stream_open_video);
    // what the library refuses — a bad format, more than 8 bits with an orientation or a reduction — is thrown with its code.
    void setVideoFormat(const acf_hip_yuv_format& fmt) { m_videoFormat = fmt; }
    const acf_hip_yuv_format& getVideoFormat() const { return m_videoFormat; }
    static Rect unorientRect(const Rect& o, int orient, int srcRows, int srcCols); // acf_hip_unorient_rect
    int acfModify(const Modify& params); // acfModify.cpp:83-152

    // Detection: planar f32 transposed image (RGB in [0,1], or LUV after setIsLuv(true)); ACF.cpp:246-265.
    // Returns 0, APPENDS to objects; scores appended (no NMS) or assigned (NMS) exactly like ACF.cpp:332-364.
    int operator()(const MatP& IpTranspose, RectVec& objects, RealVec* scores = nullptr);
    // Packed interleaved RGB f32 in [0,1], upright rows x cols x 3 unless setIsTranspose(true) (ACF.cpp:135-141).  The image is
    // copied as it is into the detector's page-locked scratch, which the device reads in place through acf_hip_run_image (this
    // library holds no HIP calls of its own, so there is no separate copy into device memory): transpose and plane split happen in
    // the ingest kernel, one pass over the host link.  With setIsTranspose(true) image rows are the array's columns and the kernel
    // takes its element-wise load form across lines of host memory: correct, but the slow way in; callers who care about speed
    // hand over upright frames, or device memory through detectImages.
    int operator()(const float* rgbInterleaved, int rows, int cols, RectVec& objects, RealVec* scores = nullptr);
    // Packed 8-bit image (CV_8UC3 RGB / CV_8UC4 / CV_8UC1 of the reference's cv::Mat entry, ACF.cpp:135-141), upright
    // rows x cols, `pix` = ACF_HIP_PIX_*, `rowStrideBytes` 0 = tight.  /255, transpose, plane split and the colour
    // conversion all happen on the device (acf_hip_run_u8).  ACF_HIP_PIX_NV12 / _NV21: a YUV 4:2:0 video frame (rows x cols luma
    // bytes, then rows / 2 rows of interleaved chroma pairs at the same stride; rows and cols even), converted as
    // cvtColor(COLOR_YUV2RGB_NV12 / _NV21) does, on the device as well (include/acf_hip.h "YUV 4:2:0 input").
    int operator()(const uint8_t* packed, int rows, int cols, int pix, int rowStrideBytes, RectVec& objects, RealVec* scores = nullptr);
    // Multi-scale search on a pyramid (ACF.cpp:268-367).
    int operator()(const Pyramid& P, RectVec& objects, RealVec* scores = nullptr);
    // Batch of frames (no reference precedent; frames are independent): per-frame outputs.
    int detectBatch(const float* framesTransposedPlanar, int nFrames, int rows, int cols, int channels,
        std::vector<RectVec>& objects, std::vector<RealVec>* scores = nullptr);

    // Batch of upright images in memory the device reads (device memory, or page-locked memory from pinnedAlloc), of any element
    // strides and element type: include/acf_hip.h, acf_hip_run_image.  rows x cols = the image's size; NMS / prune as detectBatch.
    // With setMinObjectWidth (inputScale() != 1) an ACF_HIP_T_U8 image is reduced first, in the same kernel (acf_hip_run_image_resized),
    // and the boxes are mapped back as operator()(packed) does; a float image then throws ACF_HIP_E_UNSUPPORTED.
    int detectImages(const void* framesDev, int nFrames, int rows, int cols, const acf_hip_image_desc& desc,
        std::vector<RectVec>& objects, std::vector<RealVec>* scores = nullptr);

    // Batch of YUV video frames of three planes in memory the device reads, each plane described by its own offset and byte strides
    // (I420 / YV12 / I422 / I444, packed 4:2:2, NV12 / NV21, three separately allocated planes): include/acf_hip.h, acf_hip_run_yuv.
    // The conversion is cvtColor's BT.601 integer formula (restated, parity unpinned), on the device, fused into the ingest.
    // With setMinObjectWidth (inputScale() != 1): converted, reduced and ingested in one kernel (acf_hip_run_yuv_resized), the boxes
    // mapped back as operator()(packed) does.
    int detectYuv(const uint8_t* baseDev, int nFrames, int rows, int cols, const acf_hip_yuv_desc& desc,
        std::vector<RectVec>& objects, std::vector<RealVec>* scores = nullptr);
    // After detectYuv / detectImages: the first spec.max_per_frame detections of every frame of that call, cropped out of the same
    // frames as they are stored, upright, at spec.out_h x out_w, on the device (include/acf_hip.h, acf_hip_cut_detections; kernel
    // k_cut_crops) — with the orientation, minimum object width and video format set on this object, which that call used too.
    // Exactly one of yuv / image describes the frames.  dstDev [nFrames][K][crop], boxesDev [nFrames][K][4] floats (may be null) and
    // countsDev [nFrames] int32 are device memory; the call is asynchronous and leaves them on the device: slot i of frame f is
    // detection i of the DEVICE-side list (the survivors in score order when the NMS runs on the device; a frame with more than
    // ACF_HIP_NMS_CAP detections, which detectYuv suppresses on the host, has count -1 and no crops), its box the one cv::Rect2f(o) *
    // (1.f / inputScale()) gives, in floats, grown by spec.grow.  Slots at and beyond a frame's count are not written.
    int cutDetections(const void* baseDev, int nFrames, int rows, int cols, const acf_hip_yuv_desc* yuv, const acf_hip_image_desc* image,
        const acf_hip_crop_spec& spec, void* dstDev, float* boxesDev, int32_t* countsDev);
    static size_t cropBytes(const acf_hip_crop_spec& spec, int channels); // acf_hip_crop_bytes
    // Affine views of stored frames as the batch (include/acf_hip.h, acf_hip_run_view; kernel k_ingest_view): frame i of the batch is
    // the view views[i] (six floats: xu = m0 x + m1 y + m2, yu = m3 x + m4 y + m5 from the h x w frame searched into the upright stored
    // frame) of stored frame frames[i] (frames empty: frame i) of src, samples x samples bilinear samples a pixel — one frame at a few
    // roll angles, a tracker's neighbourhood magnified, several windows of one frame.  h x w: the size searched (the plan's).  src
    // describes memory the device reads; the views and indices go through the detector's page-locked scratch.  Boxes come back in
    // VIEW coordinates: viewQuad / viewBox map one to the upright stored frame (viewBox is what acf_hip_cut_crops takes).
    int detectViews(const acf_hip_crop_source& src, const std::vector<std::array<float, 6>>& views, const std::vector<int>& frames, int samples, int h, int w,
        std::vector<RectVec>& objects, std::vector<RealVec>* scores = nullptr);
    // ... searched at the size setViewSize names, or without one at the upright stored size (acf_hip_oriented_dims of src)
    int detectViews(const acf_hip_crop_source& src, const std::vector<std::array<float, 6>>& views, const std::vector<int>& frames, int samples,
        std::vector<RectVec>& objects, std::vector<RealVec>* scores = nullptr);
    void setViewSize(int h, int w) { m_viewH = h; m_viewW = w; }
    static std::array<float, 6> viewFromBox(const std::array<float, 4>& box, double angleRad, int h, int w); // acf_hip_view_from_box
    static std::array<float, 8> viewQuad(const std::array<float, 6>& m, const Rect& o);                      // acf_hip_view_quad: TL, TR, BR, BL
    static std::array<float, 4> viewBox(const std::array<float, 6>& m, const Rect& o);                       // acf_hip_view_box
    // After detectViews: the detections of its views mapped into the upright stored frames and merged ACROSS the views of each stored
    // frame, on the device (include/acf_hip.h, acf_hip_merge_views; kernel k_merge_views) — the same object found under neighbouring
    // angles or in overlapping windows once.  views, frames: what detectViews was given; nFrames: the stored frames; spec: the NMS across
    // views, K = max_per_frame and the growth of the crop boxes.  The lists merged are the DEVICE-side ones (the per-view survivors when
    // the NMS runs on the device, else the raw lists).  merged[f].dets holds the first min(count, K) survivors of stored frame f in
    // order; merged[f].count is the true number of survivors, or -1: the frame's views hold more than ACF_HIP_NMS_CAP entries together
    // (or one of them overflowed) — there is NO host fallback for such a frame, the -1 is the answer (search fewer views of it at once,
    // or switch the per-view NMS on).  boxesDev [nFrames][K][4] floats and framesDev [nFrames][K] int32 (both or neither; memory the
    // device writes, e.g. pinnedAlloc's): every slot written, grown boxes and f in the leading slots, zeros and -1 behind them —
    // acf_hip_cut_crops(src, boxesDev, framesDev, nFrames * K, ...) is the device-only route to the crops.  Waits for the device.
    struct MergedDetection
    {
        std::array<float, 4> box;  // x, y, w, h in the upright stored frame: the bounding box of quad
        std::array<float, 8> quad; // TL, TR, BR, BL
        float score;
        int view, index;           // which view found it, and where in that view's device-side list
    };
    struct MergedFrame
    {
        std::vector<MergedDetection> dets;
        int count = 0;
    };
    int mergeViews(const std::vector<std::array<float, 6>>& views, const std::vector<int>& frames, int nFrames, const acf_hip_merge_spec& spec,
        std::vector<MergedFrame>& merged, float* boxesDev = nullptr, int32_t* framesDev = nullptr);
    // A bank of classifiers on one pyramid (include/acf_hip.h, acf_hip_set_bank / acf_hip_detect_bank / acf_hip_join_bank).  setBank:
    // up to ACF_HIP_BANK_MAX further models that share every pyramid and channel option with this detector's (checked when the model
    // next goes to the context: an Exception names the member and the field); an empty vector clears the bank.  joinBank, after any
    // detect call of nFrames frames: every member's cascade on the pyramid that call left, then the lists of the frame joined on the
    // device — model 0's RAW list (whether or not the NMS runs on the device), then the members' — under spec's NMS across the models
    // (spec.separate = 1: within each).  joined[f] holds the first min(count, K) survivors in order: boxes, scores, which model found
    // each (0: this detector's, m: member m - 1) and where in that model's device list; count is the true number, or -1: a list
    // overflowed or the frame holds more than ACF_HIP_NMS_CAP entries.  Waits for the device.
    struct Model
    {
        Options opts;
        Classifier clf;
    };
    struct BankFrame
    {
        RectVec objects;
        RealVec scores;
        std::vector<int> models, indices;
        int count = 0;
    };
    void setBank(const std::vector<Model>& members) { m_bank = members; m_dirty = true; }
    int joinBank(int nFrames, const acf_hip_bank_spec& spec, std::vector<BankFrame>& joined);
    // the descriptor of a named layout (ACF_HIP_YUV_*) of rows x cols; *frameBytes = the distance to the next frame
    static acf_hip_yuv_desc yuvLayout(int layout, int rows, int cols, int rowStrideBytes = 0, size_t* frameBytes = nullptr);
    // the same with the format's 1 or 2 bytes a sample (acf_hip_video_layout; P010 is ACF_HIP_YUV_NV12 with bits 10, shift 6)
    static acf_hip_yuv_desc videoLayout(int layout, const acf_hip_yuv_format& fmt, int rows, int cols, int rowStrideBytes = 0, size_t* frameBytes = nullptr);

    // Streaming front end (the role of GPUDetectionPipeline::runFast's two-frame FIFO, GPUDetectionPipeline.cpp:357-437):
    // batches of packed 8-bit frames are copied to the device while the previous batch computes.
    //   streamOpen(rows, cols, pix, stride, maxBatch, depth); t = streamSubmit(frames, n); streamCollect(t, objects, &scores);
    // `frames` should be page-locked (pinnedAlloc) and stay untouched until its ticket is collected; tickets are
    // collected in submission order.  At most maxDetectionsPerFrame (streamOpen) boxes per frame come back, in the
    // reference's order, before NMS/prune are applied exactly as in operator().
    void streamOpen(int rows, int cols, int pix, int rowStrideBytes, int maxBatch, int depth = 2, int maxDetectionsPerFrame = 4096);
    // the same for host frames of frameBytes each described by a YUV descriptor (acf_hip_stream_open_yuv; with setMinObjectWidth
    // acf_hip_stream_open_yuv_resized: streamCollect maps the boxes back); submit / collect as above
    void streamOpenYuv(int rows, int cols, const acf_hip_yuv_desc& desc, size_t frameBytes, int maxBatch, int depth = 2, int maxDetectionsPerFrame = 4096);
    int streamSubmit(const uint8_t* frames, int nFrames);
    // bytes from one tight frame of layout `pix` to the next: what a batch for streamSubmit / a frame for operator()(packed) holds
    static size_t u8FrameBytes(int pix, int rows, int cols, int rowStrideBytes = 0);
    void streamCollect(int ticket, std::vector<RectVec>& objects, std::vector<RealVec>* scores = nullptr);
    void streamClose();
    static void* pinnedAlloc(size_t bytes);
    static void pinnedFree(void* p);

    void computePyramid(const MatP& Ip, Pyramid& P); // ACF.cpp:147-159
    // static int Detector::chnsCompute(const MatP&, const Options::Pyramid::Chns&, Channels&, bool isInit, const MatLoggerType&)
    // (ACF.h:342-349, chnsCompute.cpp:146-338): the channels of one image at its own scale (acf_hip_chns_compute; like the
    // reference's it needs no detector — it runs on a process-wide utility context on `device`).  isInit or an empty image:
    // only chns.pChns is filled (the reference's "return the estimate", :154-198).  With a logger the planes chnsCompute logs
    // (L, U, V; M; Mnorm, O; H — tags as in :241-250, gradientMag.cpp:119-123, :285-300, :322-329) are reported: the stages
    // then run one by one through the single-operator entries, whose results are the same floats.
    static int chnsCompute(const MatP& I, const Options::Pyramid::Chns& pChns, Channels& chns, bool isInit = false, const MatLoggerType& pLogger = {},
        int device = 0);
    // static void Detector::computeChannels(const MatP& Ip, MatP& Ip2, const MatLoggerType&) (ACF.h:419-420, ACF.cpp:183-240):
    // chnsCompute with the toolbox defaults, fused into one MatP [nChns planes stacked along rows] (fuseChannels, ACF.h:653-672)
    static void computeChannels(const MatP& Ip, MatP& Ip2, const MatLoggerType& pLogger = {}, int device = 0);
    // Detector::setLogger (ACF.h:578-581): operator()(MatP) then reports every pyramid level, transposed and stretched to
    // 0..255 (cv::normalize NORM_MINMAX to 8 bits, ACF.cpp:252-262; OpenCV's rounding restated: values are whole numbers), tag "%06d"
    void setLogger(MatLoggerType logger) { m_logger = std::move(logger); }
    // Detector::setStreamLogger (ACF.h:583-586): stored; like the reference's, nothing on the hot path writes to it
    void setStreamLogger(StreamLoggerType logger) { m_streamLogger = std::move(logger); }
    // The reference's OWN arithmetic at the three sites where its SSE kernels use _mm_rsqrt_ps / _mm_rcp_ps (include/acf_hip.h,
    // option "arith"): with the tables of a CPU installed the pyramid and the detections are what the reference's compiled
    // kernels give on that CPU, bit for bit (default: exact 1/sqrt, 1/x).  setReferenceArithmetic(true) probes the CPU this
    // process runs on — "what acf::Detector would return HERE" — and throws if its instructions are not table functions;
    // the second form installs given tables (4096 + 2 x 4096 entries, acf_hip_set_x86_tables).
    void setReferenceArithmetic(bool on);
    void setReferenceArithmetic(const uint32_t* rcp4096, const uint32_t* rsqrt8192);
    static bool probeHostArithmetic(std::vector<uint32_t>& rcp4096, std::vector<uint32_t>& rsqrt8192);
    // ... and for the static chnsCompute / computeChannels (their utility context on `device`): tables, or nullptr = exact again
    static void setChnsComputeReferenceArithmetic(const uint32_t* rcp4096, const uint32_t* rsqrt8192, int device = 0);
    // chnsPyramid.cpp:160-456.  With a logger, every real scale reports the planes chnsCompute hands to its logger, in its order
    // and with its tags (chnsCompute.cpp:241-250 L,U,V; gradientMag.cpp:119-123 M; chnsCompute.cpp:285-300 Mnorm, O; :322-329 H).
    int chnsPyramid(const MatP& I, const Options::Pyramid* pPyramid, Pyramid& pyramid, bool isInit = false, const MatLoggerType& logger = {});
    // chnsPyramid.cpp:461-529; sz = {width = image height, height = image width}
    static void getScales(int nPerOct, int nOctUp, const Size& minDs, int shrink, const Size& sz,
        std::vector<double>& scales, std::vector<Size2d>& scaleshw);

    // acfDetect1.cpp:309-335: one level of fused channels ([nChns * wP rows][hP cols]) ...
    void acfDetect1(const MatP& chns, int shrink, const Size& modelDsPad, int stride, double cascThr, DetectionVec& objects);
    // ... or of an atlas plane with one roi per channel (createDetector's computeChannelIndex branch, acfDetect1.cpp:262-265,
    // 346-366): the channels are gathered into a fused buffer on the host and take the same device path
    void acfDetect1(const MatP& atlas, const RectVec& rois, int shrink, const Size& modelDsPad, int stride, double cascThr, DetectionVec& objects);
    // the same on uint8_t channels ([nChns * wP rows][hP cols] bytes), the CV_8UC1 branch of allocDetector (acfDetect1.cpp:187-192)
    void acfDetect1(const uint8_t* chnsU8, int rows, int cols, DetectionVec& objects);
    // Detector::evaluate (ACF.h:543-544, acfDetect1.cpp:337-342): score of the window at (0,0) of a fused channel buffer, trees added
    // until the score drops to 0 or below (the reference fixes cascThr = 0 for this probe)
    float evaluate(const MatP& chns, int shrink, const Size& modelDsPad, int stride);
    // float Detector::evaluate(const cv::Mat& I) const (ACF.h:543, ACF.cpp:123-133): the score of an image of the window's size —
    // computeChannels' toolbox-default channels whatever the model's Chns say, then the window at (0, 0) with cascThr 0 — on the
    // device in one call (acf_hip_evaluate_crops).  The image types operator() takes: a transposed planar MatP, or interleaved RGB
    // f32, upright unless setIsTranspose(true).  The vector forms score a batch of equally sized crops.
    float evaluate(const MatP& IpTranspose);
    float evaluate(const float* rgbInterleaved, int rows, int cols);
    std::vector<float> evaluate(const std::vector<MatP>& cropsTranspose);
    std::vector<float> evaluate(const std::vector<const float*>& rgbInterleaved, int rows, int cols);
    // ... with the channel options and cascThr of the caller's choice (pChns null: the model's own): the C entry's full argument list
    std::vector<float> evaluateCrops(const std::vector<MatP>& cropsTranspose, const Options::Pyramid::Chns* pChns, double cascThr);
    // bbNms.cpp:229-304 (max / maxg / none), ObjectDetector.cpp:28-44
    static int bbNms(const DetectionVec& bbsIn, const Options::Nms& pNms, DetectionVec& bbs);
    void prune(RectVec& objects, RealVec& scores) const;

    // Single operators (static members of acf::Detector, ACF.h:441-493), on host planes.
    int rgbConvert(const MatP& I, MatP& J, const std::string& colorSpace);
    int convTri(const MatP& I, MatP& J, double r, bool inPlaceSemantics = false);
    int gradientMag(const MatP& I, MatP& M, MatP& O, int normRad, double normConst, int full);
    int gradientHist(const MatP& M, const MatP& O, MatP& H, int binSize, int nOrients, int full, int softBin = 0); // softBin even (gradientMex.cpp:391-509)

    acf_hip_ctx* context() { return m_ctx; }

private:
    void check(int rc, const char* what) const;
    void fillParams(acf_hip_params& p) const;
    void fillParams(const Options& o, const Classifier& c, acf_hip_params& p) const; // (a bank member's: this detector's isLuv)
    void ensureContext(int device = 0); // the context, created at its first use
    void ensureModel();                 // the model on the context, pushed again after a change (m_dirty)
    void ensurePlan(int imgH, int imgW, int d, int batch);
    int numChannels() const;            // of a level, from opts.pPyramid.pChns
    // what the loggers of chnsPyramid and chnsCompute share
    static std::string planeTag(const char* name, int cols, int rows);
    static void logColourPlanes(const MatLoggerType& logger, MatP& planes, int d, int H, int W);
    static MatP hconcatHist(const float* src, int firstPlane, int nOrients, int hC, int wC);
    void fetch(int frame, RectVec& objects, RealVec* scores);
    bool resizedPlan(int rows, int cols, int& planRows, int& planCols) const;
    bool orientedPlan(int rows, int cols, bool resized, int& planRows, int& planCols) const;
    void fetchBatch(int nFrames, bool resized, std::vector<RectVec>& objects, std::vector<RealVec>* scores);
    void detect1(const float* f32, const uint8_t* u8, int rows, int cols, DetectionVec& objects);
    void finish(DetectionVec& bbs, RectVec& objects, RealVec* scores, bool forceHostNms = false) const; // ACF.cpp:332-364
    void logPyramid(); // ACF.cpp:252-262

    const hip::Api* m_api = nullptr;
    acf_hip_ctx* m_ctx = nullptr;
    bool m_good = false, m_dirty = true;
    bool m_doNms = false, m_isLuv = false, m_isTranspose = false, m_isRowMajor = false;
    void syncNms();
    bool m_nmsOnDevice = false;
    acf_hip_nms_params m_nmsSent{};
    size_t m_maxDetectionCount = 10;
    double m_detectionScorePruneRatio = 0.0;
    int m_planH = 0, m_planW = 0, m_planD = 0, m_planBatch = 0;
    std::vector<acf_hip_level> m_levels;
    int m_nChns = 0;
    std::vector<float> m_upright; // scratch for operator()(interleaved)
    int m_streamCap = 0, m_streamPix = -1, m_streamStride = 0;
    int m_orient = 0; // setInputOrientation
    int m_viewH = 0, m_viewW = 0; // setViewSize
    acf_hip_yuv_format m_videoFormat{ 8, 0, ACF_HIP_YUV_MATRIX_BT601, 0 }; // setVideoFormat
    int m_minObjectWidth = -1, m_srcRows = 0, m_srcCols = 0; // frame size handed to the 8-bit entries (== the plan's without a resize)
    MatLoggerType m_logger;
    StreamLoggerType m_streamLogger;
    bool m_taps = false; // "taps" option on: per-stage planes stay readable (needed by the logger)
    void* m_pin = nullptr; // pinned scratch of operator()(packed 8-bit)
    size_t m_pinBytes = 0;
    std::vector<Model> m_bank; // setBank's members: they go to the context with the model (ensureModel)
};

// One acf::HipDetector per visible MI355X (the north star's "batched frames shard across the GPUs of one node", host side in
// C++): detectBatch cuts the batch into contiguous blocks — the rule of acf_amd/dist.py:shard_range, blocks differ by at most
// one frame —, runs every block on its device from its own thread (frames are independent: no exchange between devices) and
// returns the per-frame results in frame order.  Setters are forwarded to every detector.
class HipDetectorPool
{
public:
    using RectVec = HipDetector::RectVec;
    using RealVec = HipDetector::RealVec;
    // devices: the device ordinals to use; empty = every visible gfx950 device (acf_hip_device_count)
    HipDetectorPool(const HipDetector::Options& o, const HipDetector::Classifier& c, std::vector<int> devices = {});
    explicit HipDetectorPool(const std::string& filename, std::vector<int> devices = {});
    size_t size() const { return m_dets.size(); }
    HipDetector& operator[](size_t i) { return *m_dets[i]; }
    static void shardRange(int nFrames, int world, int rank, int& begin, int& end);
    void setDoNonMaximaSuppression(bool f) { for (auto& d : m_dets) d->setDoNonMaximaSuppression(f); }
    void setMaxDetectionCount(size_t n) { for (auto& d : m_dets) d->setMaxDetectionCount(n); }
    void setDetectionScorePruneRatio(double r) { for (auto& d : m_dets) d->setDetectionScorePruneRatio(r); }
    void setIsLuv(bool f) { for (auto& d : m_dets) d->setIsLuv(f); }
    int acfModify(const HipDetector::Modify& m) { int rc = 0; for (auto& d : m_dets) rc |= d->acfModify(m); return rc; }
    int detectBatch(const float* framesTransposedPlanar, int nFrames, int rows, int cols, int channels,
        std::vector<RectVec>& objects, std::vector<RealVec>* scores = nullptr);

private:
    std::vector<std::unique_ptr<HipDetector>> m_dets;
};

} // namespace acf
