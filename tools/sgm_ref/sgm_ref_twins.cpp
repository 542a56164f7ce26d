/* tools/sgm_ref/sgm_ref_twins.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the three CPU twins the reference's own tests hold its kernels to (modules/cudastereo/test/test_sgm_funcs.cpp:
 * census_transform, path_aggregation, winner_takes_all_left).  Their definitions are cut out of that file at build time by
 * oracle/refshim/cu2host.py --extract into SGM_REF_TWINS_INC, which is included below; nothing of them is written here.  This file
 * gives them the little of cv::Mat they use. */
#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#define popcnt64 __builtin_popcountll
#define CV_8UC1 0
#define CV_16UC1 2
#define CV_32SC1 4

namespace cv {
struct Size {
    int width, height;
    Size(int w, int h) : width(w), height(h) {}
};
struct StereoMatcher { enum { DISP_SHIFT = 4 }; };
class Mat {   /* dense, owning or over a caller's buffer */
public:
    int rows = 0, cols = 0;
    Mat() {}
    Mat(int r, int c, int type, void *user) : rows(r), cols(c), esz_(type == CV_8UC1 ? 1 : type == CV_16UC1 ? 2 : 4), data_((unsigned char *)user) {}
    void create(Size s, int type)
    {
        rows = s.height; cols = s.width; esz_ = type == CV_8UC1 ? 1 : type == CV_16UC1 ? 2 : 4;
        own_.assign((size_t)rows * cols * esz_, 0);
        data_ = own_.data();
    }
    Size size() const { return Size(cols, rows); }
    Mat &operator=(int v) { memset(data_, v, (size_t)rows * cols * esz_); return *this; }
    template <typename T> T &at(int y, int x) { return reinterpret_cast<T *>(data_)[(size_t)y * cols + x]; }
    template <typename T> const T &at(int y, int x) const { return reinterpret_cast<const T *>(data_)[(size_t)y * cols + x]; }
    const void *bytes() const { return data_; }
    size_t nbytes() const { return (size_t)rows * cols * esz_; }
private:
    size_t esz_ = 1;
    unsigned char *data_ = nullptr;
    std::vector<unsigned char> own_;
};
}  // namespace cv

namespace opencv_test { namespace {
using namespace cv;
using std::min_element;
#include SGM_REF_TWINS_INC
}}

extern "C" {
void sgm_twin_census(const unsigned char *src, int rows, int cols, int *dst)
{
    cv::Mat s(rows, cols, CV_8UC1, (void *)src), d;
    opencv_test::census_transform(s, d);
    memcpy(dst, d.bytes(), d.nbytes());
}
void sgm_twin_path(const int *left, const int *right, int rows, int cols, int ndisp, int min_disp, int p1, int p2, int dx, int dy, unsigned char *dst)
{
    cv::Mat l(rows, cols, CV_32SC1, (void *)left), r(rows, cols, CV_32SC1, (void *)right), d;
    opencv_test::path_aggregation(l, r, d, ndisp, min_disp, p1, p2, dx, dy);
    memcpy(dst, d.bytes(), d.nbytes());
}
void sgm_twin_wta_left(const unsigned char *cost, int rows, int cols, int ndisp, int paths, float uniqueness, int subpixel, unsigned short *dst)
{
    cv::Mat c(1, paths * rows * cols * ndisp, CV_8UC1, (void *)cost), d;
    opencv_test::winner_takes_all_left(c, d, cols, rows, ndisp, paths, uniqueness, subpixel != 0);
    memcpy(dst, d.bytes(), d.nbytes());
}
}
