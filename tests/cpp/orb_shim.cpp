// Caller code written against the reference's cv::cuda::ORB (modules/cudafeatures2d/include/opencv2/cudafeatures2d.hpp:452-505) compiles
// against the drop-in header.  Without arguments it checks what needs no device and creates the object, which throws without one.  With
// two arguments (in.bin out.bin) it runs on a GPU: in.bin = rows, cols, nfeatures, nlevels (int32) + the CV_8UC1 image; out.bin = n
// (int32), the 6 x n matrix of detectAndComputeAsync, the n x 32 descriptors, then n x 6 floats of detectAndCompute's keypoints
// (x, y, size, angle, response, octave).
#include <cstdio>
#include <type_traits>
#include <vector>
#include "opencv2/cudafeatures2d.hpp"

using namespace cv;
using cuda::GpuMat;
using cuda::Stream;
typedef cuda::ORB O;

#define SAME(expr, ...) static_assert(std::is_same<decltype(expr), __VA_ARGS__>::value, #expr)
SAME(static_cast<Ptr<O> (*)(int, float, int, int, int, int, int, int, int, bool)>(&O::create), Ptr<O> (*)(int, float, int, int, int, int, int, int, int, bool));
SAME(&O::setMaxFeatures, void (O::*)(int));
SAME(&O::getMaxFeatures, int (O::*)() const);
SAME(&O::setScaleFactor, void (O::*)(double));
SAME(&O::getScaleFactor, double (O::*)() const);
SAME(&O::setNLevels, void (O::*)(int));
SAME(&O::setEdgeThreshold, void (O::*)(int));
SAME(&O::setFirstLevel, void (O::*)(int));
SAME(&O::setWTA_K, void (O::*)(int));
SAME(&O::setScoreType, void (O::*)(int));
SAME(&O::setPatchSize, void (O::*)(int));
SAME(&O::setFastThreshold, void (O::*)(int));
SAME(&O::setBlurForDescriptor, void (O::*)(bool));
SAME(&O::getBlurForDescriptor, bool (O::*)() const);
SAME(&O::descriptorSize, int (O::*)() const);
static_assert(O::X_ROW == 0 && O::Y_ROW == 1 && O::RESPONSE_ROW == 2 && O::ANGLE_ROW == 3 && O::OCTAVE_ROW == 4 && O::SIZE_ROW == 5 &&
              O::ROWS_COUNT == 6, "cudafeatures2d.hpp:455-461");
static_assert(cv::ORB::kBytes == 32 && cv::ORB::HARRIS_SCORE == 0 && cv::ORB::FAST_SCORE == 1, "cv::ORB (main repository)");
static_assert(std::is_base_of<cuda::Feature2DAsync, O>::value, "ORB is a Feature2DAsync");

static bool asserts(int wta, int patch)
{
    try { O::create(500, 1.2f, 8, 31, 0, wta, cv::ORB::HARRIS_SCORE, patch); } catch (const cv::Exception &e) { return e.code == Error::StsAssert; }
    return false;
}

int main(int argc, char **argv)
{
    try {
        if (!asserts(5, 31) || !asserts(2, 1)) return 6;   // orb.cpp:500-501: asserted before anything is created, so this needs no device
        Ptr<O> o = O::create();
        if (o->getMaxFeatures() != 500 || o->getScaleFactor() != (double)1.2f || o->getNLevels() != 8 || o->getEdgeThreshold() != 31 ||
            o->getFirstLevel() != 0 || o->getWTA_K() != 2 || o->getScoreType() != cv::ORB::HARRIS_SCORE || o->getPatchSize() != 31 ||
            o->getFastThreshold() != 20 || o->getBlurForDescriptor())
            return 2;
        if (o->descriptorSize() != 32 || o->descriptorType() != CV_8U || o->defaultNorm() != NORM_HAMMING || o->getPatternSource() != O::PATTERN_RANDOM)
            return 2;
        {   // the reference's asserts, and rejected values leave the object as it was
            bool threw = false;
            try { o->setWTA_K(5); } catch (const cv::Exception &e) { threw = e.code == Error::StsAssert; }
            if (!threw || o->getWTA_K() != 2) return 7;
            threw = false;
            try { o->setPatchSize(1); } catch (const cv::Exception &e) { threw = e.code == Error::StsAssert; }
            if (!threw || o->getPatchSize() != 31) return 7;
            threw = false;
            try { o->setNLevels(0); } catch (const cv::Exception &) { threw = true; }
            if (!threw || o->getNLevels() != 8) return 7;
            o->setWTA_K(3); o->setBlurForDescriptor(true); o->setScoreType(cv::ORB::FAST_SCORE);
            if (o->getWTA_K() != 3 || !o->getBlurForDescriptor() || o->getScoreType() != cv::ORB::FAST_SCORE) return 7;
            o->setWTA_K(2); o->setBlurForDescriptor(false); o->setScoreType(cv::ORB::HARRIS_SCORE);
        }
        if (argc < 3) return 0;
        FILE *fi = fopen(argv[1], "rb");
        int hd[4];
        if (!fi || fread(hd, 4, 4, fi) != 4) return 4;
        const int rows = hd[0], cols = hd[1];
        std::vector<unsigned char> im((size_t)rows * cols);
        if (fread(im.data(), 1, im.size(), fi) != im.size()) return 4;
        fclose(fi);
        GpuMat img(rows, cols, CV_8UC1), kp, desc, desc2;
        img.upload(im.data(), cols);
        o->setMaxFeatures(hd[2]); o->setNLevels(hd[3]);
        Stream st;
        o->detectAndComputeAsync(img, GpuMat(), kp, desc, false, st);
        const int n = kp.cols;
        if (n && (kp.rows != O::ROWS_COUNT || kp.type() != CV_32FC1 || desc.rows != n || desc.cols != 32 || desc.type() != CV_8UC1)) return 5;
        std::vector<float> mat((size_t)6 * n);
        std::vector<unsigned char> d((size_t)32 * n);
        if (n) { kp.download(mat.data(), (size_t)n * 4); desc.download(d.data(), 32); }
        std::vector<KeyPoint> a;
        o->detectAndCompute(img, GpuMat(), a, desc2);
        if ((int)a.size() != n) return 5;
        std::vector<float> flat;
        for (int i = 0; i < n; ++i) {
            const float v[6] = {a[i].pt.x, a[i].pt.y, a[i].size, a[i].angle, a[i].response, (float)a[i].octave};
            flat.insert(flat.end(), v, v + 6);
        }
        FILE *fo = fopen(argv[2], "wb");
        fwrite(&n, 4, 1, fo);
        fwrite(mat.data(), 4, mat.size(), fo);
        fwrite(d.data(), 1, d.size(), fo);
        fwrite(flat.data(), 4, flat.size(), fo);
        fclose(fo);
        return 0;
    } catch (const cv::Exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
