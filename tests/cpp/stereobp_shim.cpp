// Caller code written against the reference's cv::cuda::StereoBeliefPropagation (modules/cudastereo/include/opencv2/cudastereo.hpp:128-189)
// compiles against the drop-in header: the three compute overloads, every getter and setter, the fixed StereoMatcher getters, the
// static estimateRecommendedParams and the factory's defaults.  With two arguments (in.bin out.bin) it runs compute on a GPU:
// in.bin = rows, cols (int32) + left + right (CV_8UC1); out.bin = the CV_16SC1 disparity of compute(left, right), then of compute(data).
#include <cstdio>
#include <type_traits>
#include <vector>
#include "opencv2/cudastereo.hpp"

using namespace cv;
using cuda::GpuMat;
using cuda::Stream;
typedef cuda::StereoBeliefPropagation BP;

#define SAME(expr, ...) static_assert(std::is_same<decltype(expr), __VA_ARGS__>::value, #expr)
SAME(static_cast<void (BP::*)(cuda::InputArray, cuda::InputArray, cuda::OutputArray)>(&BP::compute), void (BP::*)(cuda::InputArray, cuda::InputArray, cuda::OutputArray));
SAME(static_cast<void (BP::*)(cuda::InputArray, cuda::InputArray, cuda::OutputArray, Stream &)>(&BP::compute),
     void (BP::*)(cuda::InputArray, cuda::InputArray, cuda::OutputArray, Stream &));
SAME(static_cast<void (BP::*)(cuda::InputArray, cuda::OutputArray, Stream &)>(&BP::compute), void (BP::*)(cuda::InputArray, cuda::OutputArray, Stream &));
SAME(&BP::estimateRecommendedParams, void (*)(int, int, int &, int &, int &));
SAME(&cuda::createStereoBeliefPropagation, Ptr<BP> (*)(int, int, int, int));
SAME(&BP::getNumIters, int (BP::*)() const);          SAME(&BP::setNumIters, void (BP::*)(int));
SAME(&BP::getNumLevels, int (BP::*)() const);         SAME(&BP::setNumLevels, void (BP::*)(int));
SAME(&BP::getMaxDataTerm, double (BP::*)() const);    SAME(&BP::setMaxDataTerm, void (BP::*)(double));
SAME(&BP::getDataWeight, double (BP::*)() const);     SAME(&BP::setDataWeight, void (BP::*)(double));
SAME(&BP::getMaxDiscTerm, double (BP::*)() const);    SAME(&BP::setMaxDiscTerm, void (BP::*)(double));
SAME(&BP::getDiscSingleJump, double (BP::*)() const); SAME(&BP::setDiscSingleJump, void (BP::*)(double));
SAME(&BP::getMsgType, int (BP::*)() const);           SAME(&BP::setMsgType, void (BP::*)(int));
static_assert(std::is_base_of<cv::StereoMatcher, BP>::value, "StereoBeliefPropagation is a cv::StereoMatcher");

int main(int argc, char **argv)
{
    int nd = 0, it = 0, lv = 0;
    try {
        BP::estimateRecommendedParams(640, 480, nd, it, lv);   // host arithmetic: needs no device
        if (nd != 160 || it != 8 || lv != 5) { fprintf(stderr, "estimateRecommendedParams: %d %d %d\n", nd, it, lv); return 2; }
        Ptr<BP> bp = cuda::createStereoBeliefPropagation();
        if (bp->getNumDisparities() != 64 || bp->getNumIters() != 5 || bp->getNumLevels() != 5 || bp->getMsgType() != CV_32F ||
            bp->getMaxDataTerm() != 10.0 || bp->getDataWeight() != (double)0.07f || bp->getMaxDiscTerm() != (double)1.7f ||
            bp->getDiscSingleJump() != 1.0 || bp->getMinDisparity() != 0 || bp->getBlockSize() != 0 || bp->getSpeckleWindowSize() != 0 ||
            bp->getSpeckleRange() != 0 || bp->getDisp12MaxDiff() != 0)
            return 2;
        if (argc < 3) return 0;
        FILE *f = fopen(argv[1], "rb");
        int dims[2];
        if (!f || fread(dims, 4, 2, f) != 2) return 4;
        const int rows = dims[0], cols = dims[1];
        std::vector<unsigned char> l((size_t)rows * cols), r(l.size());
        if (fread(l.data(), 1, l.size(), f) != l.size() || fread(r.data(), 1, r.size(), f) != r.size()) return 4;
        fclose(f);
        GpuMat left(rows, cols, CV_8UC1), right(rows, cols, CV_8UC1), disp, disp2;
        left.upload(l.data(), cols); right.upload(r.data(), cols);
        bp->setNumDisparities(16); bp->setNumIters(3); bp->setNumLevels(2); bp->setMsgType(CV_16S);
        bp->setMaxDataTerm(12.0); bp->setDataWeight(0.1); bp->setMaxDiscTerm(2.0); bp->setDiscSingleJump(0.75);
        Stream st;
        bp->compute(left, right, disp, st);
        st.waitForCompletion();
        // compute(data): a cost volume of 16 planes, each the left image's rows as shorts
        std::vector<short> vol((size_t)16 * rows * cols);
        for (int k = 0; k < 16; ++k)
            for (size_t i = 0; i < l.size(); ++i) vol[k * l.size() + i] = (short)((l[i] * (k + 1) + r[i] * (16 - k)) % 97);
        GpuMat data(16 * rows, cols, CV_MAKETYPE(CV_16S, 1));
        data.upload(vol.data(), (size_t)cols * 2);
        bp->compute(data, disp2);
        if (disp.type() != CV_MAKETYPE(CV_16S, 1) || disp2.type() != disp.type() || disp2.rows != rows || disp2.cols != cols) return 5;
        std::vector<short> out((size_t)rows * cols * 2);
        disp.download(out.data(), (size_t)cols * 2);
        disp2.download(out.data() + (size_t)rows * cols, (size_t)cols * 2);
        f = fopen(argv[2], "wb");
        fwrite(out.data(), 2, out.size(), f);
        fclose(f);
        return 0;
    } catch (const cv::Exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
