// Runs cv::superres::createSuperResolution_BTVL1_CUDA() of the drop-in header over a sequence read from a file and writes every
// output frame, so that tests/test_btvl1_gpu.py can compare the bytes with the Python mirror (both bind the same C-ABI).
//   in:  int n, rows, cols, scale, iterations, radius; then n frames of rows x cols bytes
//   out: int count, orows, ocols; then count frames of orows x ocols bytes
#include <cstdio>
#include <vector>
#include "opencv2/superres.hpp"

using namespace cv;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    try {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        int hdr[6];
        if (std::fread(hdr, sizeof(int), 6, f) != 6) return 2;
        const int n = hdr[0], rows = hdr[1], cols = hdr[2];
        std::vector<cuda::GpuMat> frames;
        std::vector<uchar> host((size_t)rows * cols);
        for (int i = 0; i < n; ++i) {
            if (std::fread(host.data(), 1, host.size(), f) != host.size()) return 2;
            cuda::GpuMat d(rows, cols, CV_8UC1);
            d.upload(host.data(), (size_t)cols);
            frames.push_back(d);
        }
        std::fclose(f);
        Ptr<superres::SuperResolution> sr = superres::createSuperResolution_BTVL1_CUDA();
        sr->setScale(hdr[3]);
        sr->setIterations(hdr[4]);
        sr->setTemporalAreaRadius(hdr[5]);
        sr->setInput(superres::createFrameSource_List(frames));
        std::vector<std::vector<uchar> > outs;
        cuda::GpuMat result;
        int orows = 0, ocols = 0;
        for (;;) {
            sr->nextFrame(result);
            if (result.empty()) break;
            if (result.type() != CV_8UC1) return 4;
            orows = result.rows; ocols = result.cols;
            outs.emplace_back((size_t)orows * ocols);
            result.download(outs.back().data(), (size_t)ocols);
        }
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        const int oh[3] = {(int)outs.size(), orows, ocols};
        std::fwrite(oh, sizeof(int), 3, o);
        for (const auto &v : outs) std::fwrite(v.data(), 1, v.size(), o);
        std::fclose(o);
    } catch (const cv::Exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
