// Compile-time check that include/opencv2/superres.hpp keeps the reference's public declarations
// (superres/include/opencv2/superres.hpp:60-203).  Shim difference, as in the optical-flow header: cv::cuda::GpuMat& stands where the
// reference has OutputArray.  Nothing here runs.
#include <type_traits>
#include "opencv2/superres.hpp"

using namespace cv;
using namespace cv::superres;

#define SAME(expr, ...) static_assert(std::is_same<decltype(expr), __VA_ARGS__>::value, #expr)
#define PROP(T, name) SAME(&SuperResolution::get##name, T (SuperResolution::*)() const); SAME(&SuperResolution::set##name, void (SuperResolution::*)(T))

// ---- superres.hpp:66-73 FrameSource
SAME(&FrameSource::nextFrame, void (FrameSource::*)(cuda::OutputArray));
SAME(&FrameSource::reset, void (FrameSource::*)());
static_assert(std::has_virtual_destructor<FrameSource>::value && std::is_abstract<FrameSource>::value, "FrameSource");
// ---- superres.hpp:75 createFrameSource_Empty
SAME(&createFrameSource_Empty, Ptr<FrameSource> (*)());

// ---- superres.hpp:87-178 SuperResolution : public cv::Algorithm, public FrameSource
static_assert(std::is_base_of<cv::Algorithm, SuperResolution>::value && std::is_base_of<FrameSource, SuperResolution>::value, "bases");
static_assert(std::is_abstract<SuperResolution>::value, "SuperResolution is an interface");
SAME(&SuperResolution::setInput, void (SuperResolution::*)(const Ptr<FrameSource> &));
SAME(&SuperResolution::nextFrame, void (SuperResolution::*)(cuda::OutputArray));
SAME(&SuperResolution::reset, void (SuperResolution::*)());
SAME(&SuperResolution::collectGarbage, void (SuperResolution::*)());
PROP(int, Scale);
PROP(int, Iterations);
PROP(double, Tau);
PROP(double, Lambda);
PROP(double, Alpha);
PROP(int, KernelSize);
PROP(int, BlurKernelSize);
PROP(double, BlurSigma);
PROP(int, TemporalAreaRadius);
SAME(&SuperResolution::getOpticalFlow, Ptr<cv::superres::DenseOpticalFlowExt> (SuperResolution::*)() const);
SAME(&SuperResolution::setOpticalFlow, void (SuperResolution::*)(const Ptr<cv::superres::DenseOpticalFlowExt> &));

// ---- superres.hpp:200 createSuperResolution_BTVL1_CUDA
SAME(&createSuperResolution_BTVL1_CUDA, Ptr<SuperResolution> (*)());

// the optical-flow factories convert to what setOpticalFlow takes (btv_l1_cuda.cpp:292)
static_assert(std::is_convertible<Ptr<FarnebackOpticalFlow>, Ptr<DenseOpticalFlowExt> >::value, "Farneback adapter");
static_assert(std::is_convertible<Ptr<DualTVL1OpticalFlow>, Ptr<DenseOpticalFlowExt> >::value, "DualTVL1 adapter");

int main() { return 0; }
