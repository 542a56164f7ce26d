/* tools/brox_ref/cu -- TEST INFRASTRUCTURE.  Texture stand-in for the recorder of cv::cuda::BroxOpticalFlow; it shadows
 * oracle/refshim/cudashim/opencv2/cudev/ptr2d/texture.hpp on the include path (nothing under oracle/ is edited) and adds the two
 * constructor forms NCVBroxOpticalFlow.cu and NPP_staging.cu use:
 *   Texture(sizeInBytes, data)                                            1-D fetch by element index: tex(i) = data[i]
 *   Texture(rows, cols, data, step, normalised, filter, address mode)     2-D read tex(y, x) with normalised coordinates
 * A texture read is DEFINED here, not measured: the CUDA programming guide's rule as the shadowed file states it (linear filtering
 * samples at x - 0.5 with the fraction in 1.8 fixed point), extended to normalised coordinates (xb = xn * W - 0.5f; point: texel
 * floor(xn * W)) and to cudaAddressModeMirror (m = k mod 2N, m < N ? m : 2N - 1 - m), every operation rounded to binary32, the four
 * products summed in the order T00, T10, T01, T11.  Written for this recorder; no reference text. */
#ifndef BROX_REF_TEXTURE_HPP
#define BROX_REF_TEXTURE_HPP
#include "opencv2/core/cuda/common.hpp"
extern "C" void brox_ref_texture_made(int rows, int cols, int linear);   /* the recorder learns the level sizes from the textures the host code makes */
static const cudaTextureAddressMode cudaAddressModeMirror = (cudaTextureAddressMode)2;
namespace cv { namespace cudev {
template <class T, class R = T> struct TexturePtr {
    const T *data = nullptr; size_t step = 0; int rows = 0, cols = 0; int linear = 0;
    static int mirror(int k, int n) { int m = k % (2 * n); if (m < 0) m += 2 * n; return m < n ? m : 2 * n - 1 - m; }
    R texel(int x, int y) const { return (R) * (const T *)((const char *)data + (size_t)mirror(y, rows) * step + (size_t)mirror(x, cols) * sizeof(T)); }
    R operator()(int i) const { return (R)data[i]; }
    R operator()(float yn, float xn) const
    {
        if (!linear) return texel((int)floorf(xn * (float)cols), (int)floorf(yn * (float)rows));
        const float xb = xn * (float)cols - 0.5f, yb = yn * (float)rows - 0.5f;
        const float fi = floorf(xb), fj = floorf(yb);
        const int i = (int)fi, j = (int)fj;
        const float a = floorf((xb - fi) * 256.0f + 0.5f) / 256.0f, b = floorf((yb - fj) * 256.0f + 0.5f) / 256.0f;
        return (R)((1.0f - a) * (1.0f - b) * texel(i, j) + a * (1.0f - b) * texel(i + 1, j) + (1.0f - a) * b * texel(i, j + 1) + a * b * texel(i + 1, j + 1));
    }
};
template <class T, class R = T> class Texture {
public:
    Texture(size_t, T *d) { p.data = d; }
    Texture(int rows, int cols, T *d, size_t step, bool, cudaTextureFilterMode f, cudaTextureAddressMode)
    {
        p.data = d; p.step = step; p.rows = rows; p.cols = cols; p.linear = f == cudaFilterModeLinear;
        brox_ref_texture_made(rows, cols, p.linear);
    }
    operator TexturePtr<T, R>() const { return p; }
private:
    TexturePtr<T, R> p;
};
}}
#endif
