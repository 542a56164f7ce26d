/* tools/stereobp_ref: in front of oracle/refshim/cudahost on the include path while modules/cudastereo/src/stereobp.cpp is compiled.
 * TEST INFRASTRUCTURE.  The stub core's OutputArray proxy lacks what StereoBPImpl::calcBP asks of it (fixedType, type, create(rows,
 * cols, type), being handed to GpuMat::convertTo) and the type code CV_16SC1: the stub's header is read with its proxy under another name, and the proxy of
 * that name is defined here on top of it. */
#ifndef SBP_REF_CORE_CUDA_HPP
#define SBP_REF_CORE_CUDA_HPP
#define _OutputArray _OutputArrayStub
#define OutputArray OutputArrayStub
#define InputOutputArray InputOutputArrayStub
#define OutputArrayOfArrays OutputArrayOfArraysStub
#define noArray noArrayStub
#include_next "opencv2/core/cuda.hpp"
#undef _OutputArray
#undef OutputArray
#undef InputOutputArray
#undef OutputArrayOfArrays
#undef noArray
#ifndef CV_16SC1
#define CV_16SC1 CV_MAKETYPE(CV_16S, 1)
#endif
namespace cv {
class _OutputArray : public _OutputArrayStub {
public:
    _OutputArray() {}
    _OutputArray(cuda::GpuMat &m, bool fixed_type = false) : _OutputArrayStub(m), fixed_(fixed_type) {}
    bool fixedType() const { return fixed_; }
    int type() const { return m_ ? m_->type() : 0; }
    using _OutputArrayStub::create;
    void create(int rows, int cols, int type) const { CV_Assert(m_); m_->create(rows, cols, type); }
    operator cuda::GpuMat &() const { CV_Assert(m_); return *m_; }
private:
    bool fixed_ = false;
};
typedef const _OutputArray &OutputArray;
typedef const _OutputArray &InputOutputArray;
typedef OutputArray OutputArrayOfArrays;
inline const _OutputArray &noArray() { static _OutputArray a; return a; }
}  // namespace cv
#endif
