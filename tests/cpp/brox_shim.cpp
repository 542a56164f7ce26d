// Caller code written against the reference's cv::cuda::BroxOpticalFlow (modules/cudaoptflow/include/opencv2/cudaoptflow.hpp:155-186) and
// cv::superres::createOptFlow_Brox_CUDA() (superres/include/opencv2/superres/optical_flow.hpp:143-177) compiles against the drop-in
// headers.  Without arguments it checks the signatures and creates the class, which throws without a device.  With two arguments
// (in.bin out.bin) it runs on a GPU: in.bin = rows, cols, inner, outer, solver (int32), alpha, gamma, scale_factor (double), the two
// CV_32FC1 frames; out.bin = rows x cols float2 of the class's calc on a stream of its own (parameters given through the setters of an
// object created with the defaults), then the u and the v plane (rows x cols floats each) of the superres adapter with its setters.
#include <cstdio>
#include <type_traits>
#include <vector>
#include "opencv2/cudaoptflow.hpp"
#include "opencv2/superres/optical_flow.hpp"

using namespace cv;
using cuda::GpuMat;
using cuda::Stream;

#define SAME(expr, ...) static_assert(std::is_same<decltype(expr), __VA_ARGS__>::value, #expr)
SAME(&cuda::BroxOpticalFlow::create, Ptr<cuda::BroxOpticalFlow> (*)(double, double, double, int, int, int));
SAME(&cuda::BroxOpticalFlow::getFlowSmoothness, double (cuda::BroxOpticalFlow::*)() const);
SAME(&cuda::BroxOpticalFlow::setGradientConstancyImportance, void (cuda::BroxOpticalFlow::*)(double));
SAME(&cuda::BroxOpticalFlow::setPyramidScaleFactor, void (cuda::BroxOpticalFlow::*)(double));
SAME(&cuda::BroxOpticalFlow::getInnerIterations, int (cuda::BroxOpticalFlow::*)() const);
SAME(&cuda::BroxOpticalFlow::setOuterIterations, void (cuda::BroxOpticalFlow::*)(int));
SAME(&cuda::BroxOpticalFlow::setSolverIterations, void (cuda::BroxOpticalFlow::*)(int));
SAME(&superres::createOptFlow_Brox_CUDA, Ptr<superres::BroxOpticalFlow> (*)());
static_assert(std::is_base_of<cuda::DenseOpticalFlow, cuda::BroxOpticalFlow>::value, "DenseOpticalFlow");
static_assert(std::is_base_of<superres::DenseOpticalFlowExt, superres::BroxOpticalFlow>::value, "DenseOpticalFlowExt");

template <class F> static int code_of(F f)
{
    try { f(); } catch (const cv::Exception &e) { return e.code; }
    return 0;
}

int main(int argc, char **argv)
{
    try {
        // rejected before a device is looked for (NCVBroxOpticalFlow.cu:606-610)
        if (code_of([] { cuda::BroxOpticalFlow::create(0.0); }) != Error::StsBadArg) return 6;
        if (code_of([] { cuda::BroxOpticalFlow::create(0.197, -1.0); }) != Error::StsBadArg) return 6;
        if (code_of([] { cuda::BroxOpticalFlow::create(0.197, 50.0, 1.0); }) != Error::StsBadArg) return 6;
        if (code_of([] { cuda::BroxOpticalFlow::create(0.197, 50.0, 0.8, 0); }) != Error::StsBadArg) return 6;
        Ptr<cuda::BroxOpticalFlow> alg = cuda::BroxOpticalFlow::create();   // the defaults; throws without a device
        if (alg->getInnerIterations() != 5 || alg->getOuterIterations() != 150 || alg->getSolverIterations() != 10) return 7;
        if (alg->getFlowSmoothness() != (double)0.197f || alg->getGradientConstancyImportance() != 50.0 || alg->getPyramidScaleFactor() != (double)0.8f) return 7;
        if (alg->getDefaultName() != "DenseOpticalFlow.BroxOpticalFlow") return 7;
        // a rejected setter leaves the object as it was
        if (code_of([&] { alg->setSolverIterations(0); }) != Error::StsBadArg || alg->getSolverIterations() != 10) return 7;
        if (code_of([&] { alg->setPyramidScaleFactor(1.5); }) != Error::StsBadArg || alg->getPyramidScaleFactor() != (double)0.8f) return 7;
        Ptr<superres::BroxOpticalFlow> ext = superres::createOptFlow_Brox_CUDA();
        if (ext->getInnerIterations() != 10 || ext->getOuterIterations() != 77 || ext->getSolverIterations() != 10) return 8;   // optical_flow.cpp:542
        if (ext->getAlpha() != (double)0.197f || ext->getGamma() != 50.0 || ext->getScaleFactor() != (double)0.8f) return 8;
        if (argc < 3) return 0;
        FILE *fi = fopen(argv[1], "rb");
        int hd[5];
        double dd[3];
        if (!fi || fread(hd, 4, 5, fi) != 5 || fread(dd, 8, 3, fi) != 3) return 4;
        const int rows = hd[0], cols = hd[1];
        std::vector<float> a((size_t)rows * cols), b(a.size());
        if (fread(a.data(), 4, a.size(), fi) != a.size() || fread(b.data(), 4, b.size(), fi) != b.size()) return 4;
        fclose(fi);
        GpuMat f0(rows, cols, CV_32FC1), f1(rows, cols, CV_32FC1), flow, u, v;
        f0.upload(a.data(), (size_t)cols * 4);
        f1.upload(b.data(), (size_t)cols * 4);
        alg->setFlowSmoothness(dd[0]); alg->setGradientConstancyImportance(dd[1]); alg->setPyramidScaleFactor(dd[2]);
        alg->setInnerIterations(hd[2]); alg->setOuterIterations(hd[3]); alg->setSolverIterations(hd[4]);
        Stream st;
        alg->calc(f0, f1, flow, st);
        st.waitForCompletion();
        if (flow.rows != rows || flow.cols != cols || flow.type() != CV_32FC2) return 5;
        std::vector<float> out((size_t)rows * cols * 2), pu(a.size()), pv(a.size());
        flow.download(out.data(), (size_t)cols * 8);
        ext->setAlpha(dd[0]); ext->setGamma(dd[1]); ext->setScaleFactor(dd[2]);
        ext->setInnerIterations(hd[2]); ext->setOuterIterations(hd[3]); ext->setSolverIterations(hd[4]);
        ext->calc(f0, f1, u, &v);
        if (u.type() != CV_32FC1 || v.type() != CV_32FC1 || u.rows != rows || v.cols != cols) return 5;
        u.download(pu.data(), (size_t)cols * 4);
        v.download(pv.data(), (size_t)cols * 4);
        ext->collectGarbage();
        FILE *fo = fopen(argv[2], "wb");
        fwrite(out.data(), 4, out.size(), fo);
        fwrite(pu.data(), 4, pu.size(), fo);
        fwrite(pv.data(), 4, pv.size(), fo);
        fclose(fo);
        return 0;
    } catch (const cv::Exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
