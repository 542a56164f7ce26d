// goodFeaturesToTrack in front of the sparse tracker, as the reference chains them (modules/videostab/src/global_motion.cpp:796-806,
// modules/cudaoptflow/test/test_optflow.cpp:203-215): cuda::createGoodFeaturesToTrackDetector finds corners on the first frame, its
// 1 x N CV_32FC2 matrix goes to cuda::SparsePyrLKOpticalFlow::calc as prevPts unchanged.  The frames are synthetic (no image codecs
// here): a texture and the same texture shifted by (2, 1) pixels, so the tracked corners should move by about (2, 1).
//   g++ -std=c++17 -Iinclude samples/track_corners.cpp -Lopencv_contrib_amd -lmiflow -Wl,-rpath,$PWD/opencv_contrib_amd -o track_corners
#include <cmath>
#include <cstdio>
#include <vector>
#include "opencv2/cudaimgproc.hpp"
#include "opencv2/cudaoptflow.hpp"

using namespace cv;

int main()
{
    try {
        const int rows = 240, cols = 320;
        std::vector<uchar> f0((size_t)rows * cols), f1(f0.size());
        auto tex = [](double x, double y) {
            return 127.5 + 60.0 * std::sin(0.31 * x + 0.5 * std::sin(0.27 * y)) + 50.0 * std::cos(0.29 * y + 0.4 * std::sin(0.25 * x));
        };
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x) {
                f0[(size_t)y * cols + x] = (uchar)std::lround(tex(x, y));
                f1[(size_t)y * cols + x] = (uchar)std::lround(tex(x - 2.0, y - 1.0));   // content moves by (+2, +1)
            }
        cuda::GpuMat d0(rows, cols, CV_8UC1), d1(rows, cols, CV_8UC1), corners, nextPts, status, err;
        d0.upload(f0.data(), cols);
        d1.upload(f1.data(), cols);

        Ptr<cuda::CornersDetector> detector = cuda::createGoodFeaturesToTrackDetector(CV_8UC1, 200, 0.01, 8.0);
        detector->detect(d0, corners);
        if (corners.empty()) { std::printf("no corners\n"); return 1; }
        const int n = corners.cols;

        Ptr<cuda::SparsePyrLKOpticalFlow> lk = cuda::SparsePyrLKOpticalFlow::create();
        lk->calc(d0, d1, corners, nextPts, status, err);

        std::vector<float> p((size_t)n * 2), q((size_t)n * 2);
        std::vector<uchar> st(n);
        corners.download(p.data(), (size_t)n * 8);
        nextPts.download(q.data(), (size_t)n * 8);
        status.download(st.data(), n);
        double su = 0, sv = 0;
        int ok = 0;
        for (int i = 0; i < n; ++i) if (st[i]) { su += q[2 * i] - p[2 * i]; sv += q[2 * i + 1] - p[2 * i + 1]; ++ok; }
        std::printf("%d corners, strongest at (%.0f, %.0f); %d tracked, mean motion (%.3f, %.3f)\n", n, p[0], p[1], ok, su / (ok ? ok : 1),
                    sv / (ok ? ok : 1));
        return 0;
    } catch (const cv::Exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
