// acf_hip_detect — C++ host CLI over acf::HipDetector (the role of the
// reference's acf-detect app, src/app/acf/acf.cpp, for this path only).
//
//   acf_hip_detect --model m.acfm --frames f.raw --rows W --cols H --channels d --count N
//                  [--luv] [--nms] [--batch] [--via-pyramid] [--max-count K] [--prune-ratio R]
//   acf_hip_detect --model m.acfm --frames f.u8 --u8 rgb|bgr|rgba|bgra|gray|nv12|nv21 --rows H --cols W --count N [--stream B] [--min-width M] ...
//                  packed 8-bit upright frames (nv12 / nv21: tight YUV 4:2:0 video frames); --stream B: batches of B frames through streamSubmit/streamCollect
//   acf_hip_detect --model m.acfm --frames f.yuv --yuv i420|yv12|i422|i444|yuyv|uyvy|yvyu|nv12|nv21 --rows H --cols W --count N [--stream B] [--min-width M]
//                  [--bits N --shift S --matrix bt601|bt709|bt2020 --range limited|full]
//                  [--orient K]
//                  tight YUV video frames of the named layout through detectYuv (one batch; the frames in page-locked memory, which the
//                  device reads), or --stream B through streamOpenYuv / streamSubmit / streamCollect; --min-width M: reduced on the device
//                  first, in the ingest kernel (acf_hip_run_yuv_resized), the boxes mapped back; --orient K (0 .. 7 = rot + 4 * mirror:
//                  the frames are stored mirrored / turned; H x W is the STORED size): the upright frame is searched
//                  (setInputOrientation), the boxes are printed in the UPRIGHT frame's coordinates and every "frame" line says so;
//                  --orient K --min-width M together: turned upright, then reduced, in one kernel (acf_hip_run_yuv_oriented_resized); the
//                  boxes are mapped back to the upright full-size frame and the "frame" line also names the reduced size;
//                  --cut WxH[:K] --cut-prefix P (without --stream): the first K detections of every frame cropped out of the stored
//                  frames on the device, upright, W x H (cutDetections), written as P_<frame>_<i>.ppm, and a "crops f n" line a frame;
//                  --view x,y,w,h[,deg[,frame]] (repeatable, without --stream) [--view-size HxW] [--view-samples s]: every view is one
//                  frame of the batch, the box of the upright stored frame turned by deg about its centre (detectViews); "view i n",
//                  then a line "x0 y0 x1 y1 x2 y2 x3 y3 score scorebits" a detection: its corners in the upright stored frame
//                  --merge OVR[:K] (with --view): the views' detections merged into their stored frames on the device (mergeViews, bbNms
//                  maxg / union / OVR across the views of a stored frame): "frame f n" per STORED frame, then up to K lines
//                  "x0 .. y3 score scorebits view index"; with --cut WxH --cut-prefix P the merged boxes' crops (acf_hip_cut_crops on
//                  mergeViews' device-side boxes) as P_<frame>_<i>.ppm and a "crops f n" line a frame.  (--cut with --view needs --merge.)
//   acf_hip_detect --model m.acfm --frames f.raw --rows W --cols H --channels d --count N --batch --also m2.acfm [--also m3.acfm ...] [--join OVR[:separate]]
//                  a bank of classifiers on one pyramid (setBank / joinBank): the frames as one batch through detectBatch, every --also
//                  model (it must share the pyramid and channel options of --model) evaluated on the same pyramid, the lists joined on the
//                  device.  "frame f n" (n: the true number of survivors, -1: unknowable), then a line "model x y w h score scorebits" a
//                  detection (model 0: --model, m: the m-th --also).  Without --join the lists concatenated, model by model; --join OVR: bbNms
//                  maxg / union / OVR across the models; --join OVR:separate: only within each model, the output in joint score order
//   acf_hip_detect --model m.acfm --frames f.raw --rows W --cols H --channels d --count N --chns out.raw [--luv] [--log-taps] [--defaults]
//                  Detector::chnsCompute per frame (static; --defaults: computeChannels' toolbox defaults instead of the model's Chns):
//                  the channels [nChns][W/shrink][H/shrink] of every frame appended to out.raw, one "chns ..." line per frame
//   acf_hip_detect --model m.acfm --frames f.raw --rows W --cols H --channels d --count N --score-crops [--defaults] [--luv]
//                  Detector::evaluate(const cv::Mat&) on the frames as one batch of crops: a "crop i score scorebits" line each
//                  (--defaults: the toolbox-default channels, as the reference; else the model's).  Without --score-crops a frame
//                  of exactly the window's size is scored the same way instead of searched (acf.cpp:350-355)
//   ... --via-images                  the same frames through detectImages: the planes described as upright images by their strides
//   ... --interleaved [--transposed]  the same frames as interleaved upright [H][W][3] images through operator()(const float*, rows, cols)
//                                     (--transposed: [W][H][3] after setIsTranspose(true))
//   ... --ref-arith host|tables.bin   the reference's rcpps / rsqrtps bits (probed from this CPU, or 4096 + 8192 uint32 from a file)
//   ... --log-levels                  Detector::setLogger: a "level <tag> <hash>" line per pyramid level
//   acf_hip_detect --convert in.acfm|in.cpb --out out.cpb                                  (model file conversion, no GPU)
//   acf_hip_detect --dump-defaults                                                         (default Options tree, no GPU)
//   acf_hip_detect --nms-only boxes.txt [--type maxg] [--overlap .65] [--ovrdnm min]   (host logic only, no GPU)
//
// Model file ("ACFHIPM1", written by acf_amd/modelio.py): text header of
// "key value" lines terminated by "END", then raw little-endian arrays
// fids u32, thrs f32, hs f32, child u32, each nTrees*nTreeNodes.
// Frames: raw f32, transposed planar [count][channels][rows=W][cols=H].
// Output: "frame i n" then n lines "x y w h score scorebits".
#include "HipDetector.h"
#include "ModelIO.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

using acf::HipDetector;

static bool loadModel(const std::string& path, HipDetector::Options& o, HipDetector::Classifier& c)
{
    return acf::loadModelAny(path, o, c) == 0; // "*.cpb": the reference's cereal files; otherwise the ACFHIPM1 container
}

static uint64_t fnv(const acf::MatP& m)
{
    uint64_t hsh = 1469598103934665603ull;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(m.data());
    for (size_t i = 0; i < m.numel() * 4; i++)
    {
        hsh = (hsh ^ b[i]) * 1099511628211ull;
    }
    return hsh;
}

static void printFrame(int f, const HipDetector::RectVec& objs, const HipDetector::RealVec& scores, const std::string& note = "")
{
    std::printf("frame %d %zu%s\n", f, objs.size(), note.c_str());
    for (size_t i = 0; i < objs.size(); i++)
    {
        const float s = float(scores[i]);
        uint32_t b;
        std::memcpy(&b, &s, 4);
        std::printf("%d %d %d %d %.9g %08x\n", objs[i].x, objs[i].y, objs[i].width, objs[i].height, scores[i], b);
    }
}

int main(int argc, char** argv)
{
    std::map<std::string, std::string> a;
    std::vector<std::string> viewArgs; // every --view, in order
    std::vector<std::string> alsoArgs; // every --also, in order
    for (int i = 1; i < argc; i++)
    {
        std::string k = argv[i];
        if (k.rfind("--", 0) == 0)
        {
            if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0)
            {
                if (k == "--view")
                {
                    viewArgs.push_back(argv[i + 1]);
                }
                if (k == "--also")
                {
                    alsoArgs.push_back(argv[i + 1]);
                }
                a[k.substr(2)] = argv[++i];
            }
            else
            {
                a[k.substr(2)] = "1";
            }
        }
    }
    try
    {
        if (a.count("nms-only"))
        {
            HipDetector::Options::Nms p;
            if (a.count("type")) p.type = a["type"];
            if (a.count("overlap")) p.overlap = std::stod(a["overlap"]);
            if (a.count("ovrdnm")) p.ovrDnm = a["ovrdnm"];
            if (a.count("thr")) p.thr = std::stod(a["thr"]);
            std::ifstream is(a["nms-only"]);
            HipDetector::DetectionVec in, out;
            HipDetector::Detection d;
            while (is >> d.roi.x >> d.roi.y >> d.roi.width >> d.roi.height >> d.score)
            {
                in.push_back(d);
            }
            HipDetector::bbNms(in, p, out);
            HipDetector det; // prune() needs only the knobs
            if (a.count("max-count")) det.setMaxDetectionCount(size_t(std::stoul(a["max-count"])));
            if (a.count("prune-ratio")) det.setDetectionScorePruneRatio(std::stod(a["prune-ratio"]));
            HipDetector::RectVec objs;
            HipDetector::RealVec scores;
            for (auto& b : out)
            {
                objs.push_back(b.roi);
                scores.push_back(b.score);
            }
            if (a.count("prune"))
            {
                det.prune(objs, scores);
            }
            printFrame(0, objs, scores);
            return 0;
        }
        HipDetector::Options o;
        HipDetector::Classifier c;
        if (a.count("dump-defaults"))
        {
            // the default Options tree (what Detector::initializeOpts / chnsCompute / chnsPyramid fill in, ACF.cpp:48-113,
            // chnsCompute.cpp:161-203, chnsPyramid.cpp:183-215): host only
            const auto& py = o.pPyramid;
            const auto& ch = py.pChns;
            std::printf("shrink %d\ncolor.enabled %d\ncolor.smooth %g\ncolor.colorSpace %s\n", ch.shrink, ch.pColor.enabled, ch.pColor.smooth, ch.pColor.colorSpace.c_str());
            std::printf("gradMag.enabled %d\ngradMag.colorChn %d\ngradMag.normRad %d\ngradMag.normConst %g\ngradMag.full %d\n", ch.pGradMag.enabled,
                ch.pGradMag.colorChn, ch.pGradMag.normRad, ch.pGradMag.normConst, ch.pGradMag.full);
            std::printf("gradHist.enabled %d\ngradHist.binSize %d\ngradHist.nOrients %d\ngradHist.softBin %d\n", ch.pGradHist.enabled, ch.pGradHist.binSize,
                ch.pGradHist.nOrients, ch.pGradHist.softBin);
            std::printf("nPerOct %d\nnOctUp %d\nnApprox %d\npad %d %d\nminDs %d %d\nsmooth %g\n", py.nPerOct, py.nOctUp, py.nApprox, py.pad.width, py.pad.height,
                py.minDs.width, py.minDs.height, py.smooth);
            std::printf("stride %d\ncascThr %g\nnms.type %s\nnms.overlap %g\nnms.ovrDnm %s\n", o.stride, o.cascThr, o.pNms.type.c_str(), o.pNms.overlap, o.pNms.ovrDnm.c_str());
            HipDetector det0;
            std::printf("maxDetectionCount 10\ngood %d\n", det0.good() ? 1 : 0);
            return 0;
        }
        if (a.count("convert"))
        {
            // acf_hip_detect --convert in.{acfm,cpb} --out out.cpb : host only
            if (!loadModel(a["convert"], o, c))
            {
                std::fprintf(stderr, "cannot read model %s\n", a["convert"].c_str());
                return 2;
            }
            std::ofstream os(a.at("out"), std::ios::binary);
            acf::saveCpb(os, o, c);
            return os ? 0 : 2;
        }
        HipDetector det(a.at("model")); // Detector(filename): "*.cpb" or the ACFHIPM1 container
        if (!det.good())
        {
            std::fprintf(stderr, "detector not good (no device / bad model)\n");
            return 3;
        }
        if ((!alsoArgs.empty() || a.count("join")) &&
            (alsoArgs.empty() || !a.count("batch") || a.count("yuv") || a.count("u8") || a.count("pool") || a.count("via-images") || a.count("interleaved") ||
                a.count("chns") || a.count("score-crops")))
        {
            throw std::runtime_error("--also / --join go with --batch on planar float frames, and --join needs an --also (said, not ignored)");
        }
        det.setIsLuv(a.count("luv") != 0);
        det.setDoNonMaximaSuppression(a.count("nms") != 0);
        if (a.count("max-count")) det.setMaxDetectionCount(size_t(std::stoul(a["max-count"])));
        if (a.count("prune-ratio")) det.setDetectionScorePruneRatio(std::stod(a["prune-ratio"]));
        if (a.count("min-width")) det.setMinObjectWidth(std::stoi(a["min-width"])); // the apps' Resizer (acf.cpp:117-148): 8-bit and YUV entries
        if (a.count("casc-cal"))
        {
            HipDetector::Modify m;
            m.has_cascCal = true;
            m.cascCal = std::stod(a["casc-cal"]);
            det.acfModify(m);
        }
        std::vector<uint32_t> arithTables;
        if (a.count("ref-arith"))
        {
            if (a["ref-arith"] == "host")
            {
                det.setReferenceArithmetic(true);
                std::vector<uint32_t> r, q;
                HipDetector::probeHostArithmetic(r, q);
                arithTables = r;
                arithTables.insert(arithTables.end(), q.begin(), q.end());
            }
            else
            {
                arithTables.resize(12288);
                std::ifstream is(a["ref-arith"], std::ios::binary);
                is.read(reinterpret_cast<char*>(arithTables.data()), 12288 * 4);
                if (!is)
                {
                    std::fprintf(stderr, "short table file\n");
                    return 2;
                }
                det.setReferenceArithmetic(arithTables.data(), arithTables.data() + 4096);
            }
        }
        if (a.count("log-levels"))
        {
            det.setLogger([](const acf::MatP& m, const std::string& t) {
                std::printf("level %s %dx%d %016llx\n", t.c_str(), m.cols(), m.rows(), static_cast<unsigned long long>(fnv(m)));
                return 0;
            });
        }
        if (a.count("yuv"))
        {
            static const std::map<std::string, int> kYuv = { { "nv12", ACF_HIP_YUV_NV12 }, { "nv21", ACF_HIP_YUV_NV21 }, { "i420", ACF_HIP_YUV_I420 },
                { "yv12", ACF_HIP_YUV_YV12 }, { "i422", ACF_HIP_YUV_I422 }, { "i444", ACF_HIP_YUV_I444 }, { "yuyv", ACF_HIP_YUV_YUYV }, { "uyvy", ACF_HIP_YUV_UYVY },
                { "yvyu", ACF_HIP_YUV_YVYU } };
            const int H = std::stoi(a.at("rows")), W = std::stoi(a.at("cols")), cnt = std::stoi(a.at("count"));
            size_t per = 0;
            // --bits N --shift S --matrix bt601|bt709|bt2020 --range limited|full: the frames' acf_hip_yuv_format (setVideoFormat)
            static const std::map<std::string, int> kMatrix = { { "bt601", ACF_HIP_YUV_MATRIX_BT601 }, { "bt709", ACF_HIP_YUV_MATRIX_BT709 },
                { "bt2020", ACF_HIP_YUV_MATRIX_BT2020 } };
            static const std::map<std::string, int> kRange = { { "limited", 0 }, { "full", 1 } };
            const acf_hip_yuv_format fmt{ a.count("bits") ? std::stoi(a["bits"]) : 8, a.count("shift") ? std::stoi(a["shift"]) : 0,
                a.count("matrix") ? kMatrix.at(a["matrix"]) : ACF_HIP_YUV_MATRIX_BT601, a.count("range") ? kRange.at(a["range"]) : 0 };
            det.setVideoFormat(fmt);
            const acf_hip_yuv_desc desc = HipDetector::videoLayout(kYuv.at(a["yuv"]), fmt, H, W, 0, &per);
            const int orient = a.count("orient") ? std::stoi(a["orient"]) : 0;
            std::string note; // what the boxes' coordinates are, when they are not the stored frame's
            if (orient)
            {
                det.setInputOrientation(orient);
                note = " upright " + std::to_string(orient & 1 ? W : H) + "x" + std::to_string(orient & 1 ? H : W) + " orient " + std::to_string(orient);
                if (det.getMinObjectWidth() >= 0 && det.inputScale() != 1.f)
                {
                    int rh = 0, rw = 0;
                    if (acf::hip::load().acf_hip_oriented_resized_dims(H, W, orient, double(det.inputScale()), &rh, &rw) == 0)
                    {
                        note += " reduced " + std::to_string(rh) + "x" + std::to_string(rw);
                    }
                }
            }
            const int B = a.count("stream") ? std::stoi(a["stream"]) : cnt, depth = 2;
            uint8_t* pin[2] = { static_cast<uint8_t*>(HipDetector::pinnedAlloc(per * size_t(B))), static_cast<uint8_t*>(HipDetector::pinnedAlloc(per * size_t(B))) };
            std::ifstream is(a.at("frames"), std::ios::binary);
            auto readBatch = [&](uint8_t* dst, int n) {
                is.read(reinterpret_cast<char*>(dst), std::streamsize(per * size_t(n)));
                if (!is)
                {
                    throw std::runtime_error("short frames file");
                }
            };
            std::vector<HipDetector::RectVec> objs;
            std::vector<HipDetector::RealVec> scores;
            if (!viewArgs.empty())
            {
                // --view x,y,w,h[,deg[,frame]] (repeatable; without --stream): every view is one frame of the batch — the box of the
                // upright stored frame `frame` (default 0) turned by deg about its centre, searched at --view-size HxW (default: the
                // upright stored size) with --view-samples s (default 1) samples a pixel each way (detectViews).  Output: "view i n",
                // then n lines "x0 y0 x1 y1 x2 y2 x3 y3 score scorebits": the detection's corners TL, TR, BR, BL in the upright stored frame
                int vh = orient & 1 ? W : H, vw = orient & 1 ? H : W, smp = a.count("view-samples") ? std::stoi(a["view-samples"]) : 1;
                if (a.count("view-size") && std::sscanf(a["view-size"].c_str(), "%dx%d", &vh, &vw) != 2)
                {
                    throw std::runtime_error("--view-size takes HxW");
                }
                std::vector<std::array<float, 6>> views;
                std::vector<int> frames;
                for (const std::string& v : viewArgs)
                {
                    float x = 0, y = 0, w = 0, h = 0;
                    double deg = 0;
                    int frame = 0;
                    if (std::sscanf(v.c_str(), "%f,%f,%f,%f,%lf,%d", &x, &y, &w, &h, &deg, &frame) < 4)
                    {
                        throw std::runtime_error("--view takes x,y,w,h[,deg[,frame]]");
                    }
                    views.push_back(HipDetector::viewFromBox({ { x, y, w, h } }, deg * 3.14159265358979323846 / 180.0, vh, vw));
                    frames.push_back(frame);
                }
                readBatch(pin[0], cnt);
                acf_hip_crop_source src{};
                src.base_dev = pin[0];
                src.n_frames = cnt;
                src.yuv = &desc;
                src.fmt = &fmt;
                src.src_rows = H;
                src.src_cols = W;
                src.orient = orient;
                det.setViewSize(vh, vw);
                if (a.count("cut") && !a.count("merge"))
                {
                    throw std::runtime_error("--cut with --view needs --merge (the views' boxes are in view coordinates)");
                }
                det.detectViews(src, views, frames, smp, objs, &scores);
                if (a.count("merge"))
                {
                    // --merge OVR[:K] (with --view): the views' detections merged into their stored frames on the device (mergeViews: bbNms
                    // "maxg" over the union with overlap OVR across the views of one stored frame, the first K (default 16) survivors a
                    // frame).  Output per STORED frame, not per view: "frame f n" (n: the survivors, -1: over capacity), then min(n, K) lines
                    // "x0 y0 x1 y1 x2 y2 x3 y3 score scorebits view index".  With --cut WxH --cut-prefix P the merged boxes are cropped out
                    // of the stored frames through mergeViews' boxes / frame indices and acf_hip_cut_crops — nothing comes to the host in
                    // between — and written as P_<frame>_<i>.ppm, a "crops f n" line a frame
                    double ovr = 0.5;
                    int K = 16;
                    if (std::sscanf(a["merge"].c_str(), "%lf:%d", &ovr, &K) < 1)
                    {
                        throw std::runtime_error("--merge takes OVR or OVR:K");
                    }
                    acf_hip_merge_spec ms{};
                    ms.nms.type = 2;
                    ms.nms.ovrDnmUnion = 1;
                    ms.nms.overlap = ovr;
                    ms.nms.thr = -1.7976931348623157e308;
                    ms.max_per_frame = K;
                    ms.grow = 1.f;
                    int cw = 0, ch = 0;
                    const bool cut = a.count("cut") != 0;
                    if (cut && std::sscanf(a["cut"].c_str(), "%dx%d", &cw, &ch) < 2)
                    {
                        throw std::runtime_error("--cut takes WxH");
                    }
                    const size_t slots = size_t(cnt) * size_t(std::max(K, 1));
                    float* boxes = cut ? static_cast<float*>(HipDetector::pinnedAlloc(slots * 4 * sizeof(float))) : nullptr;
                    int32_t* fidx = cut ? static_cast<int32_t*>(HipDetector::pinnedAlloc(slots * sizeof(int32_t))) : nullptr;
                    std::vector<HipDetector::MergedFrame> merged;
                    det.mergeViews(views, frames, cnt, ms, merged, boxes, fidx);
                    for (int f = 0; f < cnt; f++)
                    {
                        std::printf("frame %d %d\n", f, merged[size_t(f)].count);
                        for (const HipDetector::MergedDetection& d : merged[size_t(f)].dets)
                        {
                            uint32_t b;
                            std::memcpy(&b, &d.score, 4);
                            const std::array<float, 8>& q = d.quad;
                            std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %08x %d %d\n", q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], d.score, b, d.view,
                                d.index);
                        }
                    }
                    if (cut)
                    {
                        const acf_hip_crop_spec spec{ ch, cw, 1, ACF_HIP_T_U8, 1, 1, 1.f, 0 };
                        const size_t cb = HipDetector::cropBytes(spec, 3);
                        uint8_t* crops = static_cast<uint8_t*>(HipDetector::pinnedAlloc(cb * slots));
                        if (acf::hip::load().acf_hip_cut_crops(det.context(), &src, boxes, fidx, int(slots), &spec, crops) ||
                            acf::hip::load().acf_hip_synchronize(det.context()))
                        {
                            throw std::runtime_error("acf_hip_cut_crops");
                        }
                        const std::string prefix = a.count("cut-prefix") ? a["cut-prefix"] : "crop";
                        for (int f = 0; f < cnt; f++)
                        {
                            const int nc = int(merged[size_t(f)].dets.size());
                            std::printf("crops %d %d\n", f, nc);
                            for (int i = 0; i < nc; i++)
                            {
                                std::ofstream os(prefix + "_" + std::to_string(f) + "_" + std::to_string(i) + ".ppm", std::ios::binary);
                                os << "P6\n" << cw << " " << ch << "\n255\n";
                                os.write(reinterpret_cast<const char*>(crops + cb * (size_t(f) * size_t(K) + size_t(i))), std::streamsize(cb));
                            }
                        }
                        HipDetector::pinnedFree(crops);
                        HipDetector::pinnedFree(boxes);
                        HipDetector::pinnedFree(fidx);
                    }
                    HipDetector::pinnedFree(pin[0]);
                    HipDetector::pinnedFree(pin[1]);
                    return 0;
                }
                for (size_t i = 0; i < views.size(); i++)
                {
                    std::printf("view %d %d\n", int(i), int(objs[i].size()));
                    for (size_t k = 0; k < objs[i].size(); k++)
                    {
                        const std::array<float, 8> q = HipDetector::viewQuad(views[i], objs[i][k]);
                        const float sc = float(scores[i][k]);
                        uint32_t b;
                        std::memcpy(&b, &sc, 4);
                        std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %08x\n", q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], scores[i][k], b);
                    }
                }
            }
            else if (a.count("stream"))
            {
                det.streamOpenYuv(H, W, desc, per, B, depth, 8192);
                std::vector<std::pair<int, int>> inflight; // ticket, first frame
                auto drain = [&]() {
                    det.streamCollect(inflight.front().first, objs, &scores);
                    for (size_t f = 0; f < objs.size(); f++)
                    {
                        printFrame(inflight.front().second + int(f), objs[f], scores[f], note);
                    }
                    inflight.erase(inflight.begin());
                };
                int k = 0;
                for (int f0 = 0; f0 < cnt; f0 += B, k++)
                {
                    if (int(inflight.size()) == depth)
                    {
                        drain();
                    }
                    const int n = std::min(B, cnt - f0);
                    readBatch(pin[k % 2], n);
                    inflight.emplace_back(det.streamSubmit(pin[k % 2], n), f0);
                }
                while (!inflight.empty())
                {
                    drain();
                }
                det.streamClose();
            }
            else
            {
                readBatch(pin[0], cnt);
                det.detectYuv(pin[0], cnt, H, W, desc, objs, &scores);
                for (int f = 0; f < cnt; f++)
                {
                    printFrame(f, objs[size_t(f)], scores[size_t(f)], note);
                }
                if (a.count("cut"))
                {
                    // --cut WxH[:K] --cut-prefix P: the first K (default 1) detections of every frame cropped out of the stored frames on the
                    // device (cutDetections: upright, W x H, 8-bit packed R, G, B), written as P_<frame>_<i>.ppm; a "crops f n" line a frame
                    int cw = 0, ch = 0, K = 1;
                    if (std::sscanf(a["cut"].c_str(), "%dx%d:%d", &cw, &ch, &K) < 2)
                    {
                        throw std::runtime_error("--cut takes WxH or WxH:K");
                    }
                    const acf_hip_crop_spec spec{ ch, cw, 1, ACF_HIP_T_U8, 1, K, 1.f, 0 };
                    const size_t cb = HipDetector::cropBytes(spec, 3);
                    uint8_t* crops = static_cast<uint8_t*>(HipDetector::pinnedAlloc(cb * size_t(K) * size_t(cnt)));
                    int32_t* counts = static_cast<int32_t*>(HipDetector::pinnedAlloc(sizeof(int32_t) * size_t(cnt)));
                    det.cutDetections(pin[0], cnt, H, W, &desc, nullptr, spec, crops, nullptr, counts);
                    if (acf::hip::load().acf_hip_synchronize(det.context()))
                    {
                        throw std::runtime_error("acf_hip_synchronize");
                    }
                    const std::string prefix = a.count("cut-prefix") ? a["cut-prefix"] : "crop";
                    for (int f = 0; f < cnt; f++)
                    {
                        std::printf("crops %d %d\n", f, counts[f]);
                        for (int i = 0; i < counts[f]; i++)
                        {
                            std::ofstream os(prefix + "_" + std::to_string(f) + "_" + std::to_string(i) + ".ppm", std::ios::binary);
                            os << "P6\n" << cw << " " << ch << "\n255\n";
                            os.write(reinterpret_cast<const char*>(crops + cb * (size_t(f) * size_t(K) + size_t(i))), std::streamsize(cb));
                        }
                    }
                    HipDetector::pinnedFree(crops);
                    HipDetector::pinnedFree(counts);
                }
            }
            HipDetector::pinnedFree(pin[0]);
            HipDetector::pinnedFree(pin[1]);
            return 0;
        }
        if (a.count("u8"))
        {
            static const std::map<std::string, int> kPix = { { "rgb", ACF_HIP_PIX_RGB }, { "bgr", ACF_HIP_PIX_BGR }, { "rgba", ACF_HIP_PIX_RGBA },
                { "bgra", ACF_HIP_PIX_BGRA }, { "gray", ACF_HIP_PIX_GRAY }, { "nv12", ACF_HIP_PIX_NV12 }, { "nv21", ACF_HIP_PIX_NV21 } };
            const int pix = kPix.at(a["u8"]);
            const int H = std::stoi(a.at("rows")), W = std::stoi(a.at("cols")), cnt = std::stoi(a.at("count"));
            const size_t per = HipDetector::u8FrameBytes(pix, H, W);
            std::vector<uint8_t> frames(per * size_t(cnt));
            std::ifstream is(a.at("frames"), std::ios::binary);
            is.read(reinterpret_cast<char*>(frames.data()), std::streamsize(frames.size()));
            if (!is)
            {
                std::fprintf(stderr, "short frames file\n");
                return 2;
            }
            if (a.count("stream"))
            {
                const int B = std::stoi(a["stream"]), depth = 2;
                det.streamOpen(H, W, pix, 0, B, depth, 8192);
                uint8_t* pin[2] = { static_cast<uint8_t*>(HipDetector::pinnedAlloc(per * size_t(B))), static_cast<uint8_t*>(HipDetector::pinnedAlloc(per * size_t(B))) };
                std::vector<std::pair<int, int>> inflight; // ticket, first frame
                auto drain = [&]() {
                    std::vector<HipDetector::RectVec> objs;
                    std::vector<HipDetector::RealVec> scores;
                    det.streamCollect(inflight.front().first, objs, &scores);
                    for (size_t f = 0; f < objs.size(); f++)
                    {
                        printFrame(inflight.front().second + int(f), objs[f], scores[f]);
                    }
                    inflight.erase(inflight.begin());
                };
                int k = 0;
                for (int f0 = 0; f0 < cnt; f0 += B, k++)
                {
                    if (int(inflight.size()) == depth)
                    {
                        drain();
                    }
                    const int n = std::min(B, cnt - f0);
                    std::memcpy(pin[k % 2], frames.data() + per * size_t(f0), per * size_t(n));
                    inflight.emplace_back(det.streamSubmit(pin[k % 2], n), f0);
                }
                while (!inflight.empty())
                {
                    drain();
                }
                det.streamClose();
                HipDetector::pinnedFree(pin[0]);
                HipDetector::pinnedFree(pin[1]);
            }
            else
            {
                for (int f = 0; f < cnt; f++)
                {
                    HipDetector::RectVec objs;
                    HipDetector::RealVec scores;
                    det(frames.data() + per * size_t(f), H, W, pix, 0, objs, &scores);
                    printFrame(f, objs, scores);
                }
            }
            return 0;
        }
        const int rows = std::stoi(a.at("rows")), cols = std::stoi(a.at("cols")), ch = std::stoi(a.at("channels")), cnt = std::stoi(a.at("count"));
        std::vector<float> frames(size_t(rows) * cols * ch * cnt);
        {
            std::ifstream is(a.at("frames"), std::ios::binary);
            is.read(reinterpret_cast<char*>(frames.data()), std::streamsize(frames.size() * 4));
            if (!is)
            {
                std::fprintf(stderr, "short frames file\n");
                return 2;
            }
        }
        const size_t per = size_t(rows) * cols * ch;
        if (a.count("chns"))
        {
            // Detector::chnsCompute / computeChannels (static, ACF.h:342-349,419-420) on every frame
            if (!arithTables.empty())
            {
                HipDetector::setChnsComputeReferenceArithmetic(arithTables.data(), arithTables.data() + 4096);
            }
            std::ofstream os(a["chns"], std::ios::binary);
            for (int f = 0; f < cnt; f++)
            {
                acf::MatP Ip(rows, cols, ch, frames.data() + per * size_t(f));
                HipDetector::MatLoggerType logger;
                if (a.count("log-taps"))
                {
                    logger = [](const acf::MatP& m, const std::string& t) {
                        std::printf("tap %s %016llx\n", t.c_str(), static_cast<unsigned long long>(fnv(m)));
                        return 0;
                    };
                }
                if (a.count("defaults"))
                {
                    acf::MatP fused;
                    HipDetector::computeChannels(Ip, fused, logger);
                    std::printf("chns %d fused %dx%d\n", f, fused.cols(), fused.rows());
                    os.write(reinterpret_cast<const char*>(fused.data()), std::streamsize(fused.numel() * 4));
                    continue;
                }
                HipDetector::Options::Pyramid::Chns pc = det.opts.pPyramid.pChns;
                pc.isLuv = a.count("luv") != 0;
                HipDetector::Channels chns;
                HipDetector::chnsCompute(Ip, pc, chns, false, logger);
                std::printf("chns %d types %d", f, chns.nTypes);
                for (size_t t = 0; t < chns.data.size(); t++)
                {
                    std::printf(" [%s|%d|%s|%dx%d]", chns.info[t].name.c_str(), chns.info[t].nChns, chns.info[t].padWith.c_str(), chns.data[t].cols(), chns.data[t].rows());
                    os.write(reinterpret_cast<const char*>(chns.data[t].data()), std::streamsize(chns.data[t].numel() * 4));
                }
                std::printf("\n");
            }
            return os ? 0 : 2;
        }
        if (a.count("score-crops"))
        {
            // Detector::evaluate(const cv::Mat&) on every frame as ONE batch (--defaults: computeChannels' toolbox defaults, the
            // reference's method; else the model's own Chns; both with cascThr 0)
            std::vector<acf::MatP> crops;
            for (int f = 0; f < cnt; f++)
            {
                crops.emplace_back(rows, cols, ch, frames.data() + per * size_t(f));
            }
            HipDetector::Options::Pyramid::Chns pc = det.opts.pPyramid.pChns;
            pc.isLuv = a.count("luv") != 0;
            const std::vector<float> sc = a.count("defaults") ? det.evaluate(crops) : det.evaluateCrops(crops, &pc, 0.0);
            for (int f = 0; f < cnt; f++)
            {
                uint32_t b;
                std::memcpy(&b, &sc[size_t(f)], 4);
                std::printf("crop %d %.9g %08x\n", f, sc[size_t(f)], b);
            }
            return 0;
        }
        if (a.count("pool"))
        {
            // acf::HipDetectorPool: one detector per visible device ("--pool N": the first N devices, several times the same
            // device allowed through --pool-devices 0,0: contexts are independent), frames in contiguous blocks
            std::vector<int> devs;
            if (a.count("pool-devices"))
            {
                std::stringstream ss(a["pool-devices"]);
                std::string tok;
                while (std::getline(ss, tok, ','))
                {
                    devs.push_back(std::stoi(tok));
                }
            }
            acf::HipDetectorPool pool(a["model"], devs);
            pool.setIsLuv(a.count("luv") != 0);
            pool.setDoNonMaximaSuppression(a.count("nms") != 0);
            if (a.count("max-count")) pool.setMaxDetectionCount(size_t(std::stoul(a["max-count"])));
            std::vector<HipDetector::RectVec> objs;
            std::vector<HipDetector::RealVec> scores;
            pool.detectBatch(frames.data(), cnt, rows, cols, ch, objs, &scores);
            std::fprintf(stderr, "pool: %zu detector(s)\n", pool.size());
            for (int f = 0; f < cnt; f++)
            {
                printFrame(f, objs[size_t(f)], scores[size_t(f)]);
            }
        }
        else if (a.count("via-images") || a.count("interleaved"))
        {
            if (ch != 3)
            {
                std::fprintf(stderr, "--via-images / --interleaved take three planes\n");
                return 2;
            }
            // the same frames as upright images: W = rows, H = cols of the transposed planes
            const int W = rows, H = cols;
            if (a.count("via-images"))
            {
                // detectImages on the planes where they lie (in page-locked memory, which the device reads): element (c, y, x) of an
                // upright image at c * W * H + x * H + y — an image description with stride_y = 1
                float* pin = static_cast<float*>(HipDetector::pinnedAlloc(frames.size() * sizeof(float)));
                std::memcpy(pin, frames.data(), frames.size() * sizeof(float));
                acf_hip_image_desc d;
                d.dtype = ACF_HIP_T_F32;
                d.channels = 3;
                d.stride_n = int64_t(per);
                d.stride_c = int64_t(W) * H;
                d.stride_y = 1;
                d.stride_x = H;
                std::vector<HipDetector::RectVec> objs;
                std::vector<HipDetector::RealVec> scores;
                det.detectImages(pin, cnt, H, W, d, objs, &scores);
                HipDetector::pinnedFree(pin);
                for (int f = 0; f < cnt; f++)
                {
                    printFrame(f, objs[size_t(f)], scores[size_t(f)]);
                }
            }
            else
            {
                // operator()(const float* rgbInterleaved): the interleaved upright image [H][W][3] (--transposed: [W][H][3] after
                // setIsTranspose(true)) built from the planes
                const bool tr = a.count("transposed") != 0;
                det.setIsTranspose(tr);
                std::vector<float> img(per);
                for (int f = 0; f < cnt; f++)
                {
                    const float* P = frames.data() + per * size_t(f);
                    for (int z = 0; z < 3; z++)
                    {
                        for (int x = 0; x < W; x++)
                        {
                            for (int y = 0; y < H; y++)
                            {
                                const size_t px = tr ? size_t(x) * H + y : size_t(y) * W + x;
                                img[px * 3 + z] = P[(size_t(z) * W + x) * H + y];
                            }
                        }
                    }
                    HipDetector::RectVec objs;
                    HipDetector::RealVec scores;
                    det(img.data(), tr ? W : H, tr ? H : W, objs, &scores);
                    printFrame(f, objs, scores);
                }
            }
        }
        else if (a.count("batch") || !alsoArgs.empty())
        {
            if (!a.count("batch"))
            {
                throw std::runtime_error("--also needs --batch (the bank runs on the pyramid of one batch)");
            }
            std::vector<HipDetector::RectVec> objs;
            std::vector<HipDetector::RealVec> scores;
            if (!alsoArgs.empty())
            {
                std::vector<HipDetector::Model> bank(alsoArgs.size());
                for (size_t i = 0; i < alsoArgs.size(); i++)
                {
                    if (!loadModel(alsoArgs[i], bank[i].opts, bank[i].clf))
                    {
                        throw std::runtime_error("cannot read model " + alsoArgs[i]);
                    }
                }
                det.setBank(bank);
                acf_hip_bank_spec bs{};
                bs.max_per_frame = ACF_HIP_NMS_CAP;
                bs.grow = 1.f;
                if (a.count("join"))
                {
                    const std::string j = a["join"];
                    const size_t colon = j.find(':');
                    if (colon != std::string::npos && j.substr(colon + 1) != "separate")
                    {
                        throw std::runtime_error("--join takes OVR or OVR:separate");
                    }
                    bs.nms.type = 2;
                    bs.nms.ovrDnmUnion = 1;
                    bs.nms.overlap = std::stod(j.substr(0, colon));
                    bs.nms.thr = -1.7976931348623157e308;
                    bs.separate = colon != std::string::npos;
                }
                det.detectBatch(frames.data(), cnt, rows, cols, ch, objs, &scores);
                std::vector<HipDetector::BankFrame> joined;
                det.joinBank(cnt, bs, joined);
                for (int f = 0; f < cnt; f++)
                {
                    const HipDetector::BankFrame& b = joined[size_t(f)];
                    std::printf("frame %d %d\n", f, b.count);
                    for (size_t i = 0; i < b.objects.size(); i++)
                    {
                        const float sc = float(b.scores[i]);
                        uint32_t bits;
                        std::memcpy(&bits, &sc, 4);
                        std::printf("%d %d %d %d %d %.9g %08x\n", b.models[i], b.objects[i].x, b.objects[i].y, b.objects[i].width, b.objects[i].height, b.scores[i], bits);
                    }
                }
                return 0;
            }
            det.detectBatch(frames.data(), cnt, rows, cols, ch, objs, &scores);
            for (int f = 0; f < cnt; f++)
            {
                printFrame(f, objs[size_t(f)], scores[size_t(f)]);
            }
        }
        else
        {
            for (int f = 0; f < cnt; f++)
            {
                acf::MatP Ip(rows, cols, ch, frames.data() + per * size_t(f));
                HipDetector::RectVec objs;
                HipDetector::RealVec scores;
                if (a.count("log-taps"))
                {
                    // chnsPyramid with a MatLoggerType: print every tag with an FNV-1a hash of the plane's bytes
                    HipDetector::Pyramid P;
                    det.chnsPyramid(Ip, nullptr, P, true, [](const acf::MatP& m, const std::string& t) {
                        uint64_t hsh = 1469598103934665603ull;
                        const unsigned char* b = reinterpret_cast<const unsigned char*>(m.data());
                        for (size_t i = 0; i < m.numel() * 4; i++)
                        {
                            hsh = (hsh ^ b[i]) * 1099511628211ull;
                        }
                        std::printf("tap %s %016llx\n", t.c_str(), static_cast<unsigned long long>(hsh));
                        return 0;
                    });
                    continue;
                }
                if (a.count("via-atlas"))
                {
                    // the Pyramid a GL-style backend hands over: every level as ONE atlas plane with a roi per channel
                    // (ACF.h:377-378, acfDetect1.cpp:346-366): channels side by side with a gap, row stride > channel rows
                    HipDetector::Pyramid P, A;
                    det.computePyramid(Ip, P);
                    A = P;
                    A.rois.assign(size_t(P.nScales), {});
                    for (int i = 0; i < P.nScales; i++)
                    {
                        const acf::MatP& L = P.data[size_t(i)][0];
                        const int hP = L.cols(), wP = L.rows() / P.nChns;
                        // channels side by side along the atlas rows (GPUACF's texture layout): element (c, r) of channel z at
                        // c * rowStride + z * chnStride + r
                        const int chnStride = hP + 3, rowStride = P.nChns * chnStride;
                        acf::MatP view(wP, rowStride, 1);
                        std::fill(view.data(), view.data() + view.numel(), -1.f);
                        for (int z = 0; z < P.nChns; z++)
                        {
                            for (int c = 0; c < wP; c++)
                            {
                                std::memcpy(view.data() + size_t(c) * rowStride + size_t(z) * chnStride, L.data() + (size_t(z) * wP + c) * hP, sizeof(float) * hP);
                            }
                            A.rois[size_t(i)].push_back(acf::Rect(z * chnStride, 0, hP, wP));
                        }
                        A.data[size_t(i)][0] = view;
                    }
                    det(A, objs, &scores);
                }
                else if (a.count("via-pyramid"))
                {
                    // computePyramid -> host Pyramid -> another image through the detector -> operator()(Pyramid): the
                    // detections must be P's (the reference re-runs acfDetect1 on the pyramid it is handed, ACF.cpp:268-367)
                    HipDetector::Pyramid P;
                    det.computePyramid(Ip, P);
                    if (cnt > 1)
                    {
                        acf::MatP other(rows, cols, ch, frames.data() + per * size_t((f + 1) % cnt));
                        HipDetector::RectVec o2;
                        det(other, o2, nullptr);
                    }
                    det(P, objs, &scores);
                }
                else if (cols == det.getWindowSize().height && rows == det.getWindowSize().width)
                {
                    // acf.cpp:350-355: an image of exactly the window's size is scored, not searched
                    scores.push_back(det.evaluate(Ip));
                    objs.push_back(acf::Rect(0, 0, rows, cols));
                }
                else
                {
                    det(Ip, objs, &scores);
                }
                printFrame(f, objs, scores);
            }
        }
    }
    catch (const std::exception& e)
    {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
