/* tools/gftt_ref/cu: stand-in for the generated opencv2/opencv_modules.hpp: corners.cu is compiled only where cudafilters is built,
 * which makes Dx and Dy (corners.cu:53).  TEST INFRASTRUCTURE. */
#ifndef GFTT_REF_OPENCV_MODULES_HPP
#define GFTT_REF_OPENCV_MODULES_HPP
#define HAVE_OPENCV_CUDAFILTERS
#endif
