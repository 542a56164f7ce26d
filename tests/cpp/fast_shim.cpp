// Caller code written against the reference's cv::cuda::FastFeatureDetector (modules/cudafeatures2d/include/opencv2/cudafeatures2d.hpp:
// 426-442) compiles against the drop-in header, together with xfeatures2d/cuda.hpp (both name cv::KeyPoint).  Without arguments it creates
// the detector, which throws without a device.  With two arguments (in.bin out.bin) it runs on a GPU: in.bin = rows, cols, threshold,
// nonmaxSuppression, max_npoints, has_mask (int32) + the CV_8UC1 image (+ mask); out.bin = n (int32), the 2 x n matrix of detectAsync,
// then n x 5 floats of detect()'s keypoints (x, y, size, angle, response).
#include <cstdio>
#include <type_traits>
#include <vector>
#include "opencv2/cudafeatures2d.hpp"
#include "opencv2/xfeatures2d/cuda.hpp"

using namespace cv;
using cuda::GpuMat;
using cuda::Stream;
typedef cuda::FastFeatureDetector F;

#define SAME(expr, ...) static_assert(std::is_same<decltype(expr), __VA_ARGS__>::value, #expr)
SAME(&F::create, Ptr<F> (*)(int, bool, int, int));
SAME(&F::setThreshold, void (F::*)(int));
SAME(&F::setMaxNumPoints, void (F::*)(int));
SAME(&F::getMaxNumPoints, int (F::*)() const);
static_assert(F::LOCATION_ROW == 0 && F::RESPONSE_ROW == 1 && F::ROWS_COUNT == 2 && F::FEATURE_SIZE == 7, "cudafeatures2d.hpp:429-432");
static_assert(cv::FastFeatureDetector::TYPE_9_16 == 2, "cv::FastFeatureDetector::TYPE_9_16 (main repository)");
static_assert(std::is_base_of<cuda::Feature2DAsync, F>::value, "FastFeatureDetector is a Feature2DAsync");

int main(int argc, char **argv)
{
    try {
        {   // fast.cpp:213: the type is asserted before anything is created, so this needs no device
            bool threw = false;
            try { F::create(10, true, cv::FastFeatureDetector::TYPE_7_12); } catch (const cv::Exception &e) { threw = e.code == Error::StsAssert; }
            if (!threw) return 6;
        }
        Ptr<F> f = F::create();
        if (f->getThreshold() != 10 || !f->getNonmaxSuppression() || f->getMaxNumPoints() != 5000 || f->getType() != 2) return 2;
        {   // rejected values leave the object as it was
            bool threw = false;
            try { f->setThreshold(-1); } catch (const cv::Exception &) { threw = true; }
            if (!threw || f->getThreshold() != 10) return 7;
            threw = false;
            try { f->setType(cv::FastFeatureDetector::TYPE_5_8); } catch (const cv::Exception &) { threw = true; }
            if (!threw) return 7;
        }
        if (argc < 3) return 0;
        FILE *fi = fopen(argv[1], "rb");
        int hd[6];
        if (!fi || fread(hd, 4, 6, fi) != 6) return 4;
        const int rows = hd[0], cols = hd[1];
        std::vector<unsigned char> im((size_t)rows * cols), mk(hd[5] ? im.size() : 0);
        if (fread(im.data(), 1, im.size(), fi) != im.size() || fread(mk.data(), 1, mk.size(), fi) != mk.size()) return 4;
        fclose(fi);
        GpuMat img(rows, cols, CV_8UC1), mask, kp;
        img.upload(im.data(), cols);
        if (hd[5]) { mask.create(rows, cols, CV_8UC1); mask.upload(mk.data(), cols); }
        f->setThreshold(hd[2]); f->setNonmaxSuppression(hd[3] != 0); f->setMaxNumPoints(hd[4]);
        Stream st;
        f->detectAsync(img, kp, mask, st);
        const int n = kp.cols;
        if (n && (kp.rows != F::ROWS_COUNT || kp.type() != CV_32FC1)) return 5;
        std::vector<float> mat((size_t)2 * n);
        if (n) kp.download(mat.data(), (size_t)n * 4);
        std::vector<KeyPoint> a, b;
        f->detect(img, a, mask);
        f->convert(mat.data(), (size_t)n * 4, n, b);   // the host form of convert
        if ((int)a.size() != n || (int)b.size() != n) return 5;
        std::vector<float> flat;
        for (int i = 0; i < n; ++i) {
            if (a[i].pt.x != b[i].pt.x || a[i].pt.y != b[i].pt.y || a[i].response != b[i].response) return 5;
            const float v[5] = {a[i].pt.x, a[i].pt.y, a[i].size, a[i].angle, a[i].response};
            flat.insert(flat.end(), v, v + 5);
        }
        FILE *fo = fopen(argv[2], "wb");
        fwrite(&n, 4, 1, fo);
        fwrite(mat.data(), 4, mat.size(), fo);
        fwrite(flat.data(), 4, flat.size(), fo);
        fclose(fo);
        return 0;
    } catch (const cv::Exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
