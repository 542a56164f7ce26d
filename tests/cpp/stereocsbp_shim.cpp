// Caller code written against the reference's cv::cuda::StereoConstantSpaceBP (modules/cudastereo/include/opencv2/cudastereo.hpp:192-242)
// compiles against the drop-in header: the compute overloads, the getters and setters it adds to StereoBeliefPropagation, the static
// estimateRecommendedParams and the factory's defaults.  With two arguments (in.bin out.bin) it runs compute on a GPU:
// in.bin = rows, cols (int32) + left + right (CV_8UC1); out.bin = the CV_16SC1 disparity, then getNumLevels() after compute as one short.
#include <cstdio>
#include <type_traits>
#include <vector>
#include "opencv2/cudastereo.hpp"

using namespace cv;
using cuda::GpuMat;
using cuda::Stream;
typedef cuda::StereoConstantSpaceBP CS;

#define SAME(expr, ...) static_assert(std::is_same<decltype(expr), __VA_ARGS__>::value, #expr)
SAME(&CS::estimateRecommendedParams, void (*)(int, int, int &, int &, int &, int &));
SAME(&cuda::createStereoConstantSpaceBP, Ptr<CS> (*)(int, int, int, int, int));
SAME(&CS::getNrPlane, int (CS::*)() const);                SAME(&CS::setNrPlane, void (CS::*)(int));
SAME(&CS::getUseLocalInitDataCost, bool (CS::*)() const);  SAME(&CS::setUseLocalInitDataCost, void (CS::*)(bool));
static_assert(std::is_base_of<cuda::StereoBeliefPropagation, CS>::value, "StereoConstantSpaceBP is a StereoBeliefPropagation");

int main(int argc, char **argv)
{
    int nd = 0, it = 0, lv = 0, np = 0;
    try {
        CS::estimateRecommendedParams(640, 480, nd, it, lv, np);   // host arithmetic: needs no device
        if (nd != 204 || it != 10 || lv != 4 || np != 6) { fprintf(stderr, "estimateRecommendedParams: %d %d %d %d\n", nd, it, lv, np); return 2; }
        Ptr<CS> bp = cuda::createStereoConstantSpaceBP();
        if (bp->getNumDisparities() != 128 || bp->getNumIters() != 8 || bp->getNumLevels() != 4 || bp->getNrPlane() != 4 ||
            bp->getMsgType() != CV_32F || bp->getMaxDataTerm() != 30.0 || bp->getDataWeight() != 1.0 || bp->getMaxDiscTerm() != 160.0 ||
            bp->getDiscSingleJump() != 10.0 || bp->getMinDisparity() != 0 || !bp->getUseLocalInitDataCost() || bp->getBlockSize() != 0 ||
            bp->getSpeckleWindowSize() != 0 || bp->getSpeckleRange() != 0 || bp->getDisp12MaxDiff() != 0)
            return 2;
        {   // compute(data, ...) is not implemented, as in the reference (stereocsbp.cpp:331-334)
            GpuMat none, out;
            bool threw = false;
            try { bp->compute(none, out, Stream::Null()); } catch (const cv::Exception &) { threw = true; }
            if (!threw) return 6;
        }
        if (argc < 3) return 0;
        FILE *f = fopen(argv[1], "rb");
        int dims[2];
        if (!f || fread(dims, 4, 2, f) != 2) return 4;
        const int rows = dims[0], cols = dims[1];
        std::vector<unsigned char> l((size_t)rows * cols), r(l.size());
        if (fread(l.data(), 1, l.size(), f) != l.size() || fread(r.data(), 1, r.size(), f) != r.size()) return 4;
        fclose(f);
        GpuMat left(rows, cols, CV_8UC1), right(rows, cols, CV_8UC1), disp;
        left.upload(l.data(), cols); right.upload(r.data(), cols);
        bp->setNumDisparities(12); bp->setNumIters(3); bp->setNumLevels(5); bp->setNrPlane(3); bp->setMsgType(CV_16S);
        bp->setMinDisparity(1); bp->setUseLocalInitDataCost(false);
        bp->setMaxDataTerm(25.0); bp->setDataWeight(0.8); bp->setMaxDiscTerm(90.5); bp->setDiscSingleJump(7.5);
        Stream st;
        bp->compute(left, right, disp, st);
        st.waitForCompletion();
        if (disp.type() != CV_MAKETYPE(CV_16S, 1) || disp.rows != rows || disp.cols != cols) return 5;
        std::vector<short> out((size_t)rows * cols + 1);
        disp.download(out.data(), (size_t)cols * 2);
        out.back() = (short)bp->getNumLevels();
        f = fopen(argv[2], "wb");
        fwrite(out.data(), 2, out.size(), f);
        fclose(f);
        return 0;
    } catch (const cv::Exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
