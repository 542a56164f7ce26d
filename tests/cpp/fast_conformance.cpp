// Compile-time check that the drop-in cv::cuda::FastFeatureDetector keeps the reference's public signatures, transcribed from
// modules/cudafeatures2d/include/opencv2/cudafeatures2d.hpp (cited per block).  Both headers that name cv::KeyPoint are included.
// Nothing here runs.
#include <type_traits>
#include <vector>
#include "opencv2/xfeatures2d/cuda.hpp"
#include "opencv2/cudafeatures2d.hpp"

using namespace cv;
using cuda::GpuMat;
using cuda::Stream;
typedef cuda::FastFeatureDetector F;
typedef cuda::Feature2DAsync A;

#define SAME(expr, ...) static_assert(std::is_same<decltype(expr), __VA_ARGS__>::value, #expr)

// ---- cudafeatures2d.hpp:390-393 detectAsync(InputArray image, OutputArray keypoints, InputArray mask = noArray(), Stream& = Stream::Null())
SAME(&A::detectAsync, void (A::*)(cuda::InputArray, cuda::OutputArray, cuda::InputArray, Stream &));
// ---- cudafeatures2d.hpp:416-417 convert(InputArray gpu_keypoints, std::vector<KeyPoint>& keypoints)
SAME(static_cast<void (A::*)(cuda::InputArray, std::vector<KeyPoint> &)>(&A::convert), void (A::*)(cuda::InputArray, std::vector<KeyPoint> &));
// ---- cv::Feature2D::detect(InputArray image, std::vector<KeyPoint>& keypoints, InputArray mask = noArray()) (main repository), fast.cpp:71
SAME(&A::detect, void (A::*)(cuda::InputArray, std::vector<KeyPoint> &, cuda::InputArray));
// ---- cudafeatures2d.hpp:429-432
static_assert(F::LOCATION_ROW == 0 && F::RESPONSE_ROW == 1 && F::ROWS_COUNT == 2 && F::FEATURE_SIZE == 7, "the keypoint matrix");
// ---- cudafeatures2d.hpp:434-437 create(int threshold = 10, bool nonmaxSuppression = true, int type = TYPE_9_16, int max_npoints = 5000)
SAME(&F::create, Ptr<F> (*)(int, bool, int, int));
static_assert(std::is_same<decltype(F::create()), Ptr<F> >::value && std::is_same<decltype(F::create(20)), Ptr<F> >::value &&
              std::is_same<decltype(F::create(20, false)), Ptr<F> >::value && std::is_same<decltype(F::create(20, false, 2)), Ptr<F> >::value,
              "every argument of create has a default");
static_assert(cv::FastFeatureDetector::TYPE_5_8 == 0 && cv::FastFeatureDetector::TYPE_7_12 == 1 && cv::FastFeatureDetector::TYPE_9_16 == 2,
              "cv::FastFeatureDetector's types (main repository, features2d.hpp)");
// ---- cudafeatures2d.hpp:438-441
SAME(&F::setThreshold, void (F::*)(int));
SAME(&F::setMaxNumPoints, void (F::*)(int));
SAME(&F::getMaxNumPoints, int (F::*)() const);
// ---- FAST_Impl's further accessors, fast.cpp:76-86
SAME(&F::getThreshold, int (F::*)() const);
SAME(&F::setNonmaxSuppression, void (F::*)(bool));
SAME(&F::getNonmaxSuppression, bool (F::*)() const);
SAME(&F::setType, void (F::*)(int));
SAME(&F::getType, int (F::*)() const);
static_assert(std::is_base_of<A, F>::value && std::is_base_of<cv::Algorithm, A>::value && std::is_abstract<F>::value, "the class hierarchy");
// ---- cv::KeyPoint(x, y, size, angle = -1, response = 0, octave = 0, class_id = -1) (main repository, core/types.hpp), fast.cpp:205
static_assert(std::is_constructible<KeyPoint, float, float, float, float, float>::value && std::is_default_constructible<KeyPoint>::value,
              "KeyPoint's constructors");

int main() { return 0; }
