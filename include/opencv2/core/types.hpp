// The two host-side types of the main repository's opencv2/core/types.hpp that more than one drop-in header names: cv::Point2f and
// cv::KeyPoint (xfeatures2d/cuda.hpp: SURF_CUDA's keypoint vectors; cudafeatures2d.hpp: FastFeatureDetector::convert).  With real OpenCV
// headers (MIFLOW_WITH_OPENCV) the real ones are used.
#ifndef MIFLOW_OPENCV_CORE_TYPES_SHIM_HPP
#define MIFLOW_OPENCV_CORE_TYPES_SHIM_HPP

#ifndef MIFLOW_WITH_OPENCV
namespace cv {
struct Point2f { float x = 0, y = 0; };
/** opencv2/core/types.hpp KeyPoint */
struct KeyPoint {
    KeyPoint() {}
    KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0, int class_id_ = -1)
        : size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) { pt.x = x; pt.y = y; }
    Point2f pt;
    float size = 0, angle = -1, response = 0;
    int octave = 0, class_id = -1;
};
}  // namespace cv
#endif
#endif
