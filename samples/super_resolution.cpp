// BTV-L1 super-resolution through the drop-in header, in the calling pattern of the reference's own test
// (superres/test/test_superres.cpp:223-274): configure, setInput, then nextFrame until the source is exhausted.
// The reference reads a video; this tree has no videoio, so the input is a synthetic sequence of shifted, decimated frames held in
// a list-backed source.
//
//   g++ -std=c++17 -Iinclude samples/super_resolution.cpp -Lopencv_contrib_amd -lmiflow -Wl,-rpath,opencv_contrib_amd -o super_resolution
//   ./super_resolution [frames=8] [scale=2] [iterations=100] [flow=farneback|tvl1]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "opencv2/superres.hpp"

using namespace cv;

// a smooth scene with a few flat rectangles, sampled with a shift of (ox, oy) high-res pixels and decimated by `scale`
static std::vector<uchar> makeFrame(int rows, int cols, int scale, int ox, int oy)
{
    std::vector<uchar> f((size_t)rows * cols);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) {
            const double X = x * scale + ox, Y = y * scale + oy;
            double v = 128 + 60 * std::sin(X * 0.05) * std::cos(Y * 0.04) + 30 * std::sin((X + Y) * 0.11);
            if (((int)(X / 24) + (int)(Y / 18)) % 3 == 0) v = 40 + 15 * (((int)(X / 24)) % 5);
            f[(size_t)y * cols + x] = (uchar)std::min(255.0, std::max(0.0, v));
        }
    return f;
}

int main(int argc, char **argv)
{
    const int count = argc > 1 ? std::atoi(argv[1]) : 8;
    const int scale = argc > 2 ? std::atoi(argv[2]) : 2;
    const int iterations = argc > 3 ? std::atoi(argv[3]) : 100;
    const bool tvl1 = argc > 4 && !std::strcmp(argv[4], "tvl1");
    const int rows = 120, cols = 160;
    try {
        std::vector<cuda::GpuMat> frames;
        for (int i = 0; i < count; ++i) {
            const std::vector<uchar> host = makeFrame(rows, cols, scale, (i * 3) % 5 - 2, (i * 2) % 5 - 2);
            cuda::GpuMat d(rows, cols, CV_8UC1);
            d.upload(host.data(), (size_t)cols);
            frames.push_back(d);
        }

        Ptr<superres::SuperResolution> superRes = superres::createSuperResolution_BTVL1_CUDA();
        superRes->setScale(scale);
        superRes->setIterations(iterations);
        superRes->setTemporalAreaRadius(2);
        if (tvl1) superRes->setOpticalFlow(superres::createOptFlow_DualTVL1_CUDA());
        superRes->setInput(superres::createFrameSource_List(frames));

        cuda::GpuMat result;
        for (int i = 0;; ++i) {
            superRes->nextFrame(result);
            if (result.empty()) break;
            std::vector<uchar> host((size_t)result.rows * result.cols);
            result.download(host.data(), (size_t)result.cols);
            double mean = 0;
            for (uchar v : host) mean += v;
            std::printf("frame %d: %d x %d, mean %.2f\n", i, result.cols, result.rows, mean / host.size());
        }
    } catch (const cv::Exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
