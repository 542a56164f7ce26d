/* tools/fast_ref: what the reference's cudafeatures2d.hpp and fast.cpp name of the MAIN repository's opencv2/features2d.hpp (absent from
 * the reference tree): DMatch, the Feature2D base, and the two enums in the factories' defaults.  TEST INFRASTRUCTURE. */
#ifndef FAST_REF_FEATURES2D_HPP
#define FAST_REF_FEATURES2D_HPP
#include "opencv2/core/cuda.hpp"
namespace cv {
struct DMatch { int queryIdx = -1, trainIdx = -1, imgIdx = -1; float distance = 0; };
class Feature2D : public Algorithm {   /* features2d.hpp: the three virtuals the CUDA classes override */
public:
    virtual ~Feature2D() {}
    virtual void detect(InputArray, std::vector<KeyPoint> &, InputArray = noArray()) { throw std::runtime_error("not implemented"); }
    virtual void compute(InputArray, std::vector<KeyPoint> &, OutputArray) { throw std::runtime_error("not implemented"); }
    virtual void detectAndCompute(InputArray, InputArray, std::vector<KeyPoint> &, OutputArray, bool = false) { throw std::runtime_error("not implemented"); }
};
class FastFeatureDetector { public: enum { TYPE_5_8 = 0, TYPE_7_12 = 1, TYPE_9_16 = 2 }; };   /* features2d.hpp, cv::FastFeatureDetector */
class ORB { public: enum { kBytes = 32, HARRIS_SCORE = 0, FAST_SCORE = 1 }; };                  /* features2d.hpp, cv::ORB */
}
#endif
