// Caller code written against the reference's cv::cuda::CornernessCriteria / CornersDetector (modules/cudaimgproc/include/opencv2/
// cudaimgproc.hpp:535-618) compiles against the drop-in header.  Without arguments it checks what needs no device (ksize, borderType,
// the constructor's asserts) and creates the detector, which throws without a device.  With two arguments (in.bin out.bin) it runs on a
// GPU: in.bin = rows, cols, is_f32, has_mask, maxCorners, blockSize, useHarris (int32), qualityLevel, minDistance, harrisK (double), the
// image (+ CV_8UC1 mask); out.bin = n (int32) and n float2 of detect on a stream of its own, n2 and n2 float2 of a second detect on the
// same object after setMaxCorners(5) and setMinDistance(4), then the rows x cols floats of the criterion's compute.
#include <cstdio>
#include <type_traits>
#include <vector>
#include "opencv2/cudaimgproc.hpp"

using namespace cv;
using cuda::GpuMat;
using cuda::Stream;

#define SAME(expr, ...) static_assert(std::is_same<decltype(expr), __VA_ARGS__>::value, #expr)
SAME(&cuda::createHarrisCorner, Ptr<cuda::CornernessCriteria> (*)(int, int, int, double, int));
SAME(&cuda::createMinEigenValCorner, Ptr<cuda::CornernessCriteria> (*)(int, int, int, int));
SAME(&cuda::createGoodFeaturesToTrackDetector, Ptr<cuda::CornersDetector> (*)(int, int, double, double, int, bool, double));
SAME(&cuda::CornernessCriteria::compute, void (cuda::CornernessCriteria::*)(const GpuMat &, GpuMat &, Stream &));
SAME(&cuda::CornersDetector::detect, void (cuda::CornersDetector::*)(const GpuMat &, GpuMat &, const GpuMat &, Stream &));
SAME(&cuda::CornersDetector::setMaxCorners, void (cuda::CornersDetector::*)(int));
SAME(&cuda::CornersDetector::setMinDistance, void (cuda::CornersDetector::*)(double));
static_assert(std::is_base_of<Algorithm, cuda::CornersDetector>::value && std::is_base_of<Algorithm, cuda::CornernessCriteria>::value, "Algorithm");
static_assert(BORDER_REFLECT101 == 4 && BORDER_REPLICATE == 1 && BORDER_REFLECT == 2, "cv::BorderTypes (main repository)");

template <class F> static int code_of(F f)
{
    try { f(); } catch (const cv::Exception &e) { return e.code; }
    return 0;
}

int main(int argc, char **argv)
{
    try {
        // rejected before a device is looked for
        if (code_of([] { cuda::createMinEigenValCorner(CV_8UC1, 3, 5); }) != Error::StsNotImplemented) return 6;
        if (code_of([] { cuda::createHarrisCorner(CV_8UC1, 3, -1, 0.04); }) != Error::StsNotImplemented) return 6;
        if (code_of([] { cuda::createHarrisCorner(CV_8UC1, 3, 3, 0.04, BORDER_WRAP); }) != Error::StsBadArg) return 6;    // corners.cpp:86
        if (code_of([] { cuda::createGoodFeaturesToTrackDetector(CV_8UC1, 1000, 0.0); }) != Error::StsBadArg) return 6;   // gftt.cpp:94
        if (code_of([] { cuda::createGoodFeaturesToTrackDetector(CV_8UC1, -1); }) != Error::StsBadArg) return 6;
        if (code_of([] { cuda::createGoodFeaturesToTrackDetector(CV_8UC1, 1000, 0.01, -1.0); }) != Error::StsBadArg) return 6;
        Ptr<cuda::CornersDetector> det = cuda::createGoodFeaturesToTrackDetector(CV_8UC1);   // the defaults; throws without a device
        if (code_of([&] { det->setMaxCorners(-1); }) != Error::StsBadArg || code_of([&] { det->setMinDistance(-1); }) != Error::StsBadArg) return 7;
        if (argc < 3) return 0;
        FILE *fi = fopen(argv[1], "rb");
        int hd[7];
        double dd[3];
        if (!fi || fread(hd, 4, 7, fi) != 7 || fread(dd, 8, 3, fi) != 3) return 4;
        const int rows = hd[0], cols = hd[1], type = hd[2] ? CV_32FC1 : CV_8UC1;
        const size_t es = hd[2] ? 4 : 1;
        std::vector<unsigned char> im((size_t)rows * cols * es), mk(hd[3] ? (size_t)rows * cols : 0);
        if (fread(im.data(), 1, im.size(), fi) != im.size() || fread(mk.data(), 1, mk.size(), fi) != mk.size()) return 4;
        fclose(fi);
        GpuMat img(rows, cols, type), mask, corners, plane;
        img.upload(im.data(), cols * es);
        if (hd[3]) { mask.create(rows, cols, CV_8UC1); mask.upload(mk.data(), cols); }
        det = cuda::createGoodFeaturesToTrackDetector(type, hd[4], dd[0], dd[1], hd[5], hd[6] != 0, dd[2]);
        FILE *fo = fopen(argv[2], "wb");
        Stream st;
        for (int pass = 0; pass < 2; ++pass) {
            if (pass) { det->setMaxCorners(5); det->setMinDistance(4.0); }
            det->detect(img, corners, mask, st);   // waits for the stream itself
            const int n = corners.cols;
            if (n && (corners.rows != 1 || corners.type() != CV_32FC2)) return 5;
            if (!n && !corners.empty()) return 5;
            std::vector<float> pts((size_t)2 * n);
            if (n) corners.download(pts.data(), pts.size() * 4);
            fwrite(&n, 4, 1, fo);
            fwrite(pts.data(), 4, pts.size(), fo);
        }
        Ptr<cuda::CornernessCriteria> crit = hd[6] ? cuda::createHarrisCorner(type, hd[5], 3, dd[2]) : cuda::createMinEigenValCorner(type, hd[5], 3);
        crit->compute(img, plane, st);
        st.waitForCompletion();
        if (plane.rows != rows || plane.cols != cols || plane.type() != CV_32FC1) return 5;
        std::vector<float> pl((size_t)rows * cols);
        plane.download(pl.data(), (size_t)cols * 4);
        fwrite(pl.data(), 4, pl.size(), fo);
        fclose(fo);
        return 0;
    } catch (const cv::Exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
