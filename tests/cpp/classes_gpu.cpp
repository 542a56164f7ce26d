// Caller code against the drop-in headers alone: StereoSGM, DisparityBilateralFilter, DensePyrLKOpticalFlow, SparsePyrLKOpticalFlow and
// DescriptorMatcher, run through their public C++ classes on a GPU.  tests/test_cpp_classes_gpu.py writes the inputs, runs
//     classes_gpu <sgm|dbf|dense|sparse|bf|params> in.bin out.bin
// and compares what the classes return with the oracle.  Both files are a flat sequence of records
//     int32 name length, type (CV_MAKETYPE code), rows, cols; the name; rows * cols elements, dense
// Every output a class creates itself is a GpuMat::create matrix (pitched rows when rows > 1); where a case asks for it the output is
// a Rect view inside a larger matrix filled with the byte 0xA5, and the whole larger matrix is written too.  A cv::Exception a case
// raises is recorded as the array "<case>.exc" holding its code.  Without a device: exit status 3.
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "opencv2/cudafeatures2d.hpp"
#include "opencv2/cudaoptflow.hpp"
#include "opencv2/cudastereo.hpp"
#include "opencv2/xfeatures2d/cuda.hpp"

using namespace cv;
using cuda::GpuMat;
using cuda::Stream;
typedef std::vector<std::vector<DMatch> > Lists;

struct Arr {
    int type = 0, rows = 0, cols = 0;
    std::vector<uchar> b;
    const int *i() const { return reinterpret_cast<const int *>(b.data()); }
    const float *f() const { return reinterpret_cast<const float *>(b.data()); }
    const int *row(int r) const { return i() + (size_t)r * cols; }
};
static std::map<std::string, Arr> in;
static FILE *out = nullptr;

static size_t esz(int type)
{
    static const int sz[8] = {1, 1, 2, 2, 4, 4, 8, 2};
    return (size_t)sz[CV_MAT_DEPTH(type)] * CV_MAT_CN(type);
}
static std::string num(int v) { return std::to_string(v); }

static bool load(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int h[4];
    bool ok = true;
    while (ok && fread(h, 4, 4, f) == 4) {
        std::string name((size_t)h[0], '\0');
        Arr a;
        a.type = h[1]; a.rows = h[2]; a.cols = h[3];
        a.b.resize((size_t)a.rows * a.cols * esz(a.type));
        ok = fread(&name[0], 1, name.size(), f) == name.size() && (a.b.empty() || fread(a.b.data(), 1, a.b.size(), f) == a.b.size());
        in[name] = a;
    }
    fclose(f);
    return ok;
}
static const Arr &arr(const std::string &name)
{
    auto it = in.find(name);
    if (it == in.end()) throw std::runtime_error("no input array " + name);
    return it->second;
}
static void put(const std::string &name, int type, int rows, int cols, const void *data)
{
    const int h[4] = {(int)name.size(), type, rows, cols};
    fwrite(h, 4, 4, out);
    fwrite(name.data(), 1, name.size(), out);
    if (rows > 0 && cols > 0) fwrite(data, esz(type), (size_t)rows * cols, out);
}
static void puti(const std::string &name, const std::vector<int> &v) { put(name, CV_32SC1, 1, (int)v.size(), v.data()); }
static void put(const std::string &name, const GpuMat &m)
{
    std::vector<uchar> h((size_t)m.rows * m.cols * m.elemSize());
    if (!m.empty()) m.download(h.data(), (size_t)m.cols * m.elemSize());
    put(name, m.type(), m.rows, m.cols, h.data());
}
static GpuMat up(const std::string &name)
{
    const Arr &a = arr(name);
    GpuMat m(a.rows, a.cols, a.type);
    if (!m.empty()) m.upload(a.b.data(), (size_t)a.cols * esz(a.type));
    return m;
}
template <class F> static void guarded(const std::string &name, F f)
{
    try { f(); } catch (const cv::Exception &e) { puti(name + ".exc", {e.code}); }
}

// a rows x cols view at (3, 2) of a matrix 7 columns and 5 rows larger, every byte of which is 0xA5
struct Framed {
    GpuMat big, view;
    const uchar *data0 = nullptr;
    Framed(int rows, int cols, int type)
    {
        big.create(rows + 5, cols + 7, type);
        big.setTo(0xA5);
        view = big(Rect(3, 2, cols, rows));
        data0 = view.data;
    }
    void write(const std::string &name) const
    {
        put(name, view);
        put(name + ".big", big);
        puti(name + ".inplace", {view.data == data0 && view.step == big.step && view.refcount == big.refcount});
    }
};
// form 0: the output is an empty GpuMat; form 1: a sentinel-framed view of the right size and type
template <class F> static void runOut(const std::string &name, int form, int rows, int cols, int type, F call)
{
    if (form == 0) {
        GpuMat o;
        call(o);
        put(name, o);
        puti(name + ".step", {(int)o.step});
    } else {
        Framed f(rows, cols, type);
        call(f.view);
        f.write(name);
    }
}

// cases: frame, minDisparity, numDisparities, P1, P2, uniquenessRatio, mode, form, how (0: a new object from all arguments, 1: a new
// object createStereoSGM(minDisparity, numDisparities), 2: the object of the case before, through its setters)
static void sgm()
{
    const Arr &c = arr("cases");
    Ptr<cuda::StereoSGM> alg;
    GpuMat l, r;
    for (int i = 0; i < c.rows; ++i) {
        const int *p = c.row(i);
        l = up("l" + num(p[0])); r = up("r" + num(p[0]));
        if (p[8] == 0) alg = cuda::createStereoSGM(p[1], p[2], p[3], p[4], p[5], p[6]);
        else if (p[8] == 1) alg = cuda::createStereoSGM(p[1], p[2]);
        else {
            alg->setMinDisparity(p[1]); alg->setNumDisparities(p[2]); alg->setP1(p[3]); alg->setP2(p[4]); alg->setUniquenessRatio(p[5]);
            alg->setMode(p[6]);
        }
        puti("out" + num(i) + ".params", {alg->getMinDisparity(), alg->getNumDisparities(), alg->getP1(), alg->getP2(), alg->getUniquenessRatio(),
                                         alg->getMode()});
        guarded("out" + num(i), [&] {
            runOut("out" + num(i), p[7], l.rows, l.cols, CV_MAKETYPE(CV_16S, 1), [&](GpuMat &o) { alg->compute(l, r, o); });
        });
    }
    // a value the class rejects: the setters store it like the reference's, compute() throws, and after the old value is back the
    // object computes what it computed before
    const int nd = alg->getNumDisparities();
    int setterThrew = 0, computeThrew = 0;
    try { alg->setNumDisparities(96); } catch (const cv::Exception &) { setterThrew = 1; }
    try { GpuMat o; alg->compute(l, r, o); } catch (const cv::Exception &e) { computeThrew = e.code; }
    try { alg->setNumDisparities(nd); } catch (const cv::Exception &) { setterThrew |= 2; }
    puti("reject", {setterThrew, computeThrew, alg->getNumDisparities()});
    Stream st;
    GpuMat again;
    alg->compute(l, r, again, st);
    st.waitForCompletion();
    put("again", again);
}

// cases: disparity array, image array, ndisp, radius, iters, setters (1: the three thresholds are set after construction), form (0, 1,
// or 2: dst is the disparity matrix itself)
static void dbf()
{
    const Arr &c = arr("cases");
    for (int i = 0; i < c.rows; ++i) {
        const int *p = c.row(i);
        const std::string n = "out" + num(i);
        GpuMat d = up("disp" + num(p[0])), img = up("img" + num(p[1]));
        Ptr<cuda::DisparityBilateralFilter> f = cuda::createDisparityBilateralFilter(p[2], p[3], p[4]);
        if (p[5]) { f->setEdgeThreshold(0.05); f->setMaxDiscThreshold(0.3); f->setSigmaRange(25.0); }
        guarded(n, [&] {
            if (p[6] == 2) {
                const uchar *d0 = d.data;
                Stream st;
                f->apply(d, img, d, st);
                st.waitForCompletion();
                put(n, d);
                puti(n + ".inplace", {d.data == d0});
            } else
                runOut(n, p[6], d.rows, d.cols, d.type(), [&](GpuMat &o) { f->apply(d, img, o); });
        });
    }
}

// cases: frame, window width, window height, maxLevel, iters, useInitialFlow, form
static void dense()
{
    const Arr &c = arr("cases");
    for (int i = 0; i < c.rows; ++i) {
        const int *p = c.row(i);
        GpuMat a = up("a" + num(p[0])), b = up("b" + num(p[0]));
        Ptr<cuda::DensePyrLKOpticalFlow> alg = cuda::DensePyrLKOpticalFlow::create(Size(p[1], p[2]), p[3], p[4], p[5] != 0);
        guarded("out" + num(i), [&] {
            runOut("out" + num(i), p[6], a.rows, a.cols, CV_32FC2, [&](GpuMat &o) { alg->calc(a, b, o); });
        });
    }
}

// cases: frame, N, maxLevel, err requested, useInitialFlow (2: with a nextPts of N + 1 points), form; one object runs them all
static void sparse()
{
    const Arr &c = arr("cases");
    Ptr<cuda::SparsePyrLKOpticalFlow> alg = cuda::SparsePyrLKOpticalFlow::create(Size(9, 9), 3, 10);
    auto run = [&](const int *p, const std::string &n) {
        const int N = p[1];
        GpuMat a = up("a" + num(p[0])), b = up("b" + num(p[0])), pts = up("pts" + num(N));
        alg->setMaxLevel(p[2]);
        alg->setUseInitialFlow(p[4] != 0);
        Framed fn(1, N ? N : 4, CV_32FC2), fs(1, N ? N : 4, CV_8UC1), fe(1, N ? N : 4, CV_32FC1);
        GpuMat nxt, st, err;
        if (p[5] || N == 0) { nxt = fn.view; st = fs.view; err = fe.view; }   // N = 0: non-empty outputs that the class has to release
        if (p[4] == 1) {
            if (!p[5]) nxt.create(1, N, CV_32FC2);
            nxt.upload(arr("init" + num(N)).b.data(), (size_t)N * 8);
        }
        if (p[4] == 2) { nxt = GpuMat(1, N + 1, CV_32FC2); nxt.setTo(0); }
        if (p[3]) {
            Stream stream;
            alg->calc(a, b, pts, nxt, st, err, stream);
            stream.waitForCompletion();
        } else {
            // the caller's err matrix, filled by a call that asks for it, is not an argument of the call that does not
            if (N) {
                alg->calc(a, b, pts, nxt, st, err);
                put(n + ".err1", err);
            }
            const uchar *e0 = err.data;
            alg->calc(a, b, pts, nxt, st);
            puti(n + ".errkept", {err.data == e0});
        }
        if (N == 0) { puti(n + ".released", {nxt.empty(), st.empty(), err.empty()}); return; }
        if (p[5]) { fn.write(n + ".next"); fs.write(n + ".status"); fe.write(n + ".err"); }
        else { put(n + ".next", nxt); put(n + ".status", st); put(n + ".err", err); }
        puti(n + ".steps", {(int)nxt.step, (int)st.step, (int)err.step});
    };
    for (int i = 0; i < c.rows; ++i) guarded("out" + num(i), [&] { run(c.row(i), "out" + num(i)); });
    // a window the library rejects: the setter throws, the getter still answers the old window and the next call runs with it
    int threw = 0;
    try { alg->setWinSize(Size(2, 21)); } catch (const cv::Exception &e) { threw = e.code; }
    puti("reject", {threw, alg->getWinSize().width, alg->getWinSize().height});
    guarded("again", [&] { run(c.row(c.rows - 1), "again"); });
}

static void putMatches(const std::string &name, const std::vector<DMatch> &m)
{
    std::vector<int> v;
    for (const DMatch &d : m) {
        int bits;
        std::memcpy(&bits, &d.distance, 4);
        v.push_back(d.queryIdx); v.push_back(d.trainIdx); v.push_back(d.imgIdx); v.push_back(bits);
    }
    put(name, CV_32SC1, (int)m.size(), 4, v.data());
}
static void putLists(const std::string &name, const Lists &ls)
{
    std::vector<DMatch> flat;
    std::vector<int> len;
    for (const std::vector<DMatch> &l : ls) { len.push_back((int)l.size()); flat.insert(flat.end(), l.begin(), l.end()); }
    putMatches(name, flat);
    puti(name + ".len", len);
}

// norm, nsets; per set s<i>.: q, t (the train matrix), t0 and t1 (the two add() calls of the collection), mask (q x t), m0 and m1 (the
// collection's masks), ks (the list lengths), radii.  Every form runs on the train matrix (tg 0) and on the collection (tg 1), without a
// mask (mk 0), with the masks (mk 1; once more with compactResult) and, for the collection, with an empty GpuMat as the first mask
// (mk 2); directly (.d) and as *Async on a stream of its own followed by *Convert (.a), whose packed matrix is written as .raw.
static void bf()
{
    const int norm = arr("norm").i()[0], nsets = arr("nsets").i()[0];
    for (int s = 0; s < nsets; ++s) {
        const std::string S = "s" + num(s) + ".";
        const GpuMat q = up(S + "q"), t = up(S + "t"), mask = up(S + "mask");
        const std::vector<GpuMat> t0(1, up(S + "t0")), t1(1, up(S + "t1"));
        std::vector<GpuMat> cm[3];
        cm[1].push_back(up(S + "m0")); cm[1].push_back(up(S + "m1"));
        cm[2].push_back(GpuMat()); cm[2].push_back(cm[1][1]);
        const Arr &ks = arr(S + "ks"), &radii = arr(S + "radii");
        Stream stream;
        Ptr<cuda::DescriptorMatcher> single = cuda::DescriptorMatcher::createBFMatcher(norm), coll = cuda::DescriptorMatcher::createBFMatcher(norm);
        coll->add(t0);
        coll->add(t1);
        puti(S + "coll", {(int)coll->getTrainDescriptors().size(), coll->empty(), single->empty(), coll->isMaskSupported()});
        for (int tg = 0; tg < 2; ++tg)
            for (int mk = 0; mk < (tg ? 3 : 2); ++mk)
                for (int c = 0; c < (mk == 1 ? 2 : 1); ++c) {
                    const std::string V = "." + num(tg) + num(mk) + num(c);
                    const GpuMat m1 = mk ? mask : GpuMat();
                    const bool compact = c != 0;
                    std::string n;
                    if (!c) {
                        guarded(n = S + "match.d" + V, [&] {
                            std::vector<DMatch> r;
                            if (tg) coll->match(q, r, cm[mk]); else single->match(q, t, r, m1);
                            putMatches(n, r);
                        });
                        guarded(n = S + "match.a" + V, [&] {
                            GpuMat g;
                            std::vector<DMatch> r;
                            if (tg) coll->matchAsync(q, g, cm[mk], stream); else single->matchAsync(q, t, g, m1, stream);
                            stream.waitForCompletion();
                            single->matchConvert(g, r);
                            putMatches(n, r);
                            put(S + "match.raw" + V, g);
                        });
                    }
                    for (int j = 0; j < ks.cols; ++j) {
                        const int k = ks.i()[j];
                        guarded(n = S + "knn" + num(k) + ".d" + V, [&] {
                            Lists r;
                            if (tg) coll->knnMatch(q, r, k, cm[mk], compact); else single->knnMatch(q, t, r, k, m1, compact);
                            putLists(n, r);
                        });
                        guarded(n = S + "knn" + num(k) + ".a" + V, [&] {
                            GpuMat g;
                            Lists r;
                            if (tg) coll->knnMatchAsync(q, g, k, cm[mk], stream); else single->knnMatchAsync(q, t, g, k, m1, stream);
                            stream.waitForCompletion();
                            single->knnMatchConvert(g, r, compact);
                            putLists(n, r);
                            if (!c) put(S + "knn" + num(k) + ".raw" + V, g);
                        });
                    }
                    for (int j = 0; j < radii.cols; ++j) {
                        const float radius = radii.f()[j];
                        guarded(n = S + "rad" + num(j) + ".d" + V, [&] {
                            Lists r;
                            if (tg) coll->radiusMatch(q, r, radius, cm[mk], compact); else single->radiusMatch(q, t, r, radius, m1, compact);
                            putLists(n, r);
                        });
                        guarded(n = S + "rad" + num(j) + ".a" + V, [&] {
                            GpuMat g;
                            Lists r;
                            if (tg) coll->radiusMatchAsync(q, g, radius, cm[mk], stream); else single->radiusMatchAsync(q, t, g, radius, m1, stream);
                            stream.waitForCompletion();
                            single->radiusMatchConvert(g, r, compact);
                            putLists(n, r);
                            if (!c) put(S + "rad" + num(j) + ".raw" + V, g);
                        });
                    }
                }
        coll->clear();
        puti(S + "cleared", {coll->empty()});
    }
    if (in.count("xq")) {   // the calls that must throw
        const GpuMat xq = up("xq"), xt = up("xt"), q = up("s0.q"), t = up("s0.t");
        guarded("x.hamming_f32", [&] {
            std::vector<DMatch> r;
            cuda::DescriptorMatcher::createBFMatcher(NORM_HAMMING)->match(xq, xt, r);
            puti("x.hamming_f32", {(int)r.size()});
        });
        guarded("x.k17", [&] {
            Lists r;
            cuda::DescriptorMatcher::createBFMatcher(norm)->knnMatch(q, t, r, 17);
            puti("x.k17", {(int)r.size()});
        });
        guarded("x.coll_async_k3", [&] {
            Ptr<cuda::DescriptorMatcher> m = cuda::DescriptorMatcher::createBFMatcher(norm);
            m->add(std::vector<GpuMat>(1, t));
            GpuMat g;
            m->knnMatchAsync(q, g, 3);
            puti("x.coll_async_k3", {g.rows});
        });
    }
}

// A value the library's set_params rejects, for the two classes whose set_params validates: the setter throws, the getter still answers
// the old value, another setter with a valid value succeeds, and the object then computes what a new object with the same final
// parameters computes.  Then SURF_CUDA's error path: a call the library refuses before any launch leaves the caller's descriptors
// header as it was.
static void params()
{
    GpuMat a = up("a"), b = up("b"), pts = up("pts");
    {
        Ptr<cuda::OpticalFlowDual_TVL1> alg = cuda::OpticalFlowDual_TVL1::create(0.25, 0.15, 0.3, 3, 2, 0.01, 20);
        int threw = 0;
        try { alg->setNumScales(0); } catch (const cv::Exception &e) { threw = e.code; }
        const int kept = alg->getNumScales();
        alg->setNumWarps(3);
        puti("tvl1.reject", {threw, kept, alg->getNumScales(), alg->getNumWarps()});
        GpuMat f0, f1;
        alg->calc(a, b, f0);
        cuda::OpticalFlowDual_TVL1::create(0.25, 0.15, 0.3, 3, 3, 0.01, 20)->calc(a, b, f1);
        put("tvl1.kept", f0); put("tvl1.fresh", f1);
    }
    {
        Ptr<cuda::SparsePyrLKOpticalFlow> alg = cuda::SparsePyrLKOpticalFlow::create(Size(9, 9), 2, 10);
        int threw = 0;
        try { alg->setMaxLevel(16); } catch (const cv::Exception &e) { threw = e.code; }
        const int kept = alg->getMaxLevel();
        alg->setNumIters(7);
        puti("sparse.reject", {threw, kept, alg->getMaxLevel(), alg->getNumIters()});
        GpuMat n0, s0, n1, s1;
        alg->calc(a, b, pts, n0, s0);
        cuda::SparsePyrLKOpticalFlow::create(Size(9, 9), 2, 7)->calc(a, b, pts, n1, s1);
        put("sparse.kept.next", n0); put("sparse.kept.status", s0); put("sparse.fresh.next", n1); put("sparse.fresh.status", s1);
    }
    {
        cuda::SURF_CUDA surf(arr("surf").f()[0], 2, 2, false, arr("surf").f()[1]);
        GpuMat kp, desc, wrong(a.rows, a.cols, CV_32FC1);
        wrong.setTo(0);
        surf(a, GpuMat(), kp, desc);                  // desc: an allocation of maxFeatures rows, cut to the feature count
        const int rows0 = desc.rows, cols0 = desc.cols;
        const uchar *data0 = desc.data;
        const int maxf = (int)((desc.dataend - desc.datastart - (size_t)cols0 * 4) / desc.step) + 1;
        int threw = 0;
        try { surf(wrong, GpuMat(), kp, desc); } catch (const cv::Exception &e) { threw = e.code; }   // MI_ERR_BAD_TYPE before any launch
        puti("surf.reject", {threw, rows0, cols0, maxf, desc.rows, desc.cols, desc.data == data0});
    }
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: classes_gpu <sgm|dbf|dense|sparse|bf|params> in.bin out.bin\n"); return 2; }
    try {
        if (cuda::getCudaEnabledDeviceCount() < 1) {
            fprintf(stderr, "classes_gpu: no GPU device, and the library has no CPU fallback\n");
            return 3;
        }
        if (!load(argv[2])) { fprintf(stderr, "classes_gpu: cannot read %s\n", argv[2]); return 4; }
        out = fopen(argv[3], "wb");
        if (!out) { fprintf(stderr, "classes_gpu: cannot write %s\n", argv[3]); return 4; }
        const std::string family = argv[1];
        if (family == "sgm") sgm();
        else if (family == "dbf") dbf();
        else if (family == "dense") dense();
        else if (family == "sparse") sparse();
        else if (family == "bf") bf();
        else if (family == "params") params();
        else { fprintf(stderr, "classes_gpu: no family %s\n", argv[1]); return 2; }
        return fclose(out) == 0 ? 0 : 4;
    } catch (const cv::Exception &e) {
        fprintf(stderr, "classes_gpu: cv::Exception %d: %s\n", e.code, e.what());
        return e.code == Error::GpuNotSupported ? 3 : 5;
    } catch (const std::exception &e) {
        fprintf(stderr, "classes_gpu: %s\n", e.what());
        return 6;
    }
}
