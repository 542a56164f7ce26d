/* tools/gftt_ref/cu: in front of oracle/refshim/cudavec's border_interpolate.hpp while the reference's cudaimgproc/src/cuda/corners.cu
 * is compiled for the host.  TEST INFRASTRUCTURE.  Adds what corners.cu asks of the main repository and the stand-ins lack: the names of
 * the three border modes its launch wrappers switch on (cv::BorderTypes, core/base.hpp) and the wait of a stream (everything runs on the
 * calling thread here).  The index maps are oracle/refshim/cudavec's, unchanged. */
#ifndef GFTT_REF_BORDER_INTERPOLATE_HPP
#define GFTT_REF_BORDER_INTERPOLATE_HPP
#include_next "opencv2/core/cuda/border_interpolate.hpp"
namespace cv { enum { BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_REFLECT_101 = 4, BORDER_REFLECT101 = 4 }; }
#ifndef GFTT_REF_HAVE_STREAM_SYNC
#define GFTT_REF_HAVE_STREAM_SYNC
static inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }
#endif
#endif
