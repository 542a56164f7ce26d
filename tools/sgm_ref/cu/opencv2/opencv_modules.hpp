/* tools/sgm_ref/cu: opencv2/opencv_modules.hpp of a build with cudev (modules/cudastereo/src/cuda/stereosgm.cu compiles its body only
 * then).  TEST INFRASTRUCTURE. */
#ifndef SGM_REF_OPENCV_MODULES_HPP
#define SGM_REF_OPENCV_MODULES_HPP
#define HAVE_OPENCV_CUDEV
#endif
