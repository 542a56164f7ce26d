// Band height of the streaming TV-L1 kernels (csrc/tvl1_plan.h tb_band_rows): the band COUNT is the round-3 rule's, the height is the
// one that minimises the summed executed steps of the bands among the heights that cut that many bands, keep the floor of 8 rows and
// make no band run more blocks than the tallest band of the equal cut does.  Checked against an independent restatement of the
// round-3 rule and a brute force over every height.  Plain C++, no device.
#include "tvl1_plan.h"
#include <cstdio>

using namespace mi::tvl1;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
static long long wave_steps(int T, int PF, int rows) { const int P = T + 1 + PF; return ceil_div(rows + 2 * T, P) * P; }

// the round-3 rule as plan_band_rows stated it (tvl1_tbr_kernels.hip before round 20): -> band count
static int old_band_count(int T, int PF, int H, long long per_band, long long cap, long long simds, int wps)
{
    long long best_cost = -1;
    int best_nb = 1;
    for (int nb = 1; nb <= H; ++nb) {
        const int R = (int)ceil_div(H, nb);
        if (R < 8 && nb > 1) break;
        const long long cap_nb = simds > 0 && nb < 4 && nb < wps ? simds * nb : cap;
        const long long rounds = ceil_div(per_band * nb, cap_nb);
        const long long cost = rounds * wave_steps(T, PF, R);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_nb = nb; }
    }
    return best_nb;
}
// summed steps of the bands a kernel launched with `R` rows per band runs: bands [k R, min((k + 1) R, H))
static long long sum_steps(int T, int PF, int H, int R)
{
    long long s = 0;
    for (int y0 = 0; y0 < H; y0 += R) s += wave_steps(T, PF, (y0 + R < H ? y0 + R : H) - y0);
    return s;
}

static void check_one(int T, int PF, int H, long long per_band, long long cap, long long simds, int wps)
{
    const TbBandShape b{T, PF, H, per_band, cap, simds, wps};
    const int nb = old_band_count(T, PF, H, per_band, cap, simds, wps);
    const int R0 = (int)ceil_div(H, nb);
    const int R = tb_band_rows(b);
    CHECK(tb_band_count(b) == nb);
    CHECK(tb_band_rows_equal(b) == R0);
    CHECK(ceil_div(H, R) == nb);                         // the band count is the old rule's
    CHECK(R >= 8 || nb == 1);
    CHECK(R >= 1 && R <= H);
    CHECK(sum_steps(T, PF, H, R) <= sum_steps(T, PF, H, R0));
    CHECK(wave_steps(T, PF, R) <= wave_steps(T, PF, R0));   // no band runs longer than the tallest band of the equal cut
    CHECK(tb_band_sum_steps(T, PF, H, R) == sum_steps(T, PF, H, R));
    // brute force over every height: the minimum over the admissible ones, the smallest such height
    long long best = -1;
    int best_R = -1;
    for (int r = 1; r <= H; ++r) {
        if (ceil_div(H, r) != nb || (r < 8 && nb > 1) || wave_steps(T, PF, r) > wave_steps(T, PF, R0)) continue;
        const long long s = sum_steps(T, PF, H, r);
        if (best < 0 || s < best) { best = s; best_R = r; }
    }
    CHECK(best >= 0 && sum_steps(T, PF, H, R) == best && R == best_R);
    if (fails) std::printf("  at T=%d PF=%d H=%d per_band=%lld cap=%lld simds=%lld wps=%d: nb=%d R0=%d R=%d\n", T, PF, H, per_band, cap, simds, wps, nb, R0, R);
}

// waves per band row of the joined-wave T = 10 kernel (256-column strips with a margin of 10 columns at the outer edges, four waves)
static long long jw_per_band(int w, int pairs) { return (w <= 246 ? 1 : 1 + ceil_div(w - 246, 236)) * pairs * 4; }

int main()
{
    // sweep: heights 16 .. 2200, waves per band row from one strip of one pair to 1080p x 64 pairs, capacities of 2 .. 8 waves per
    // SIMD of 1024 SIMDs and of a small device, joined (simds = 0) and independent waves
    for (int T : {1, 2, 3, 4, 5, 6, 8, 10})
        for (int PF : {1, 2})
            for (int H = 16; H <= 2200; H += (H < 200 ? 1 : 7))
                for (long long per_band : {1ll, 4ll, 44ll, 352ll, 528ll, 1056ll, 2816ll})
                    for (int wps : {2, 3, 4, 8})
                        for (long long simds : {1024ll, 64ll}) {
                            check_one(T, PF, H, per_band, simds * wps, 0, wps);
                            check_one(T, PF, H, per_band, simds * wps, simds, wps);
                            if (fails) { std::printf("tvl1_band_test: FAILED\n"); return 1; }
                        }
    // every height 16 .. 2200 at the headline's kernel
    for (int H = 16; H <= 2200; ++H)
        for (int pairs : {1, 8, 16, 32}) check_one(10, 2, H, jw_per_band(1920, pairs), 3072, 0, 3);

    // the headline's five levels at 32 pairs per lane (T = 10, PF = 2, three waves per SIMD of 1024 SIMDs): 553 rows 3 x 148 + 109 = 637
    // steps instead of 4 x 139 = 663, 442 rows 5 x 82 + 32 = 572 instead of 6 x 74 = 624, nothing to gain at 1080, 864 and 691 rows
    struct Ex { int w, h, pairs, R0, R; long long s0, s; };
    const Ex ex[] = {{1920, 1080, 32, 135, 135, 8 * 156, 8 * 156}, {1536, 864, 32, 288, 288, 3 * 312, 3 * 312}, {1229, 691, 32, 173, 173, 4 * 195, 4 * 195},
                     {983, 553, 32, 139, 148, 663, 637}, {786, 442, 32, 74, 82, 624, 572},
                     // 16 pairs per lane: 1080 rows 1 183 instead of 1 235 steps
                     {1920, 1080, 16, 216, -1, 1235, 1183}};
    for (const Ex &e : ex) {
        const TbBandShape b{10, 2, e.h, jw_per_band(e.w, e.pairs), 3072, 0, 3};
        CHECK(tb_band_rows_equal(b) == e.R0);
        CHECK(sum_steps(10, 2, e.h, e.R0) == e.s0);
        const int R = tb_band_rows(b);
        CHECK(e.R < 0 || R == e.R);
        CHECK(sum_steps(10, 2, e.h, R) == e.s);
        if (fails) std::printf("  example %dx%d x %d: R0=%d R=%d sum0=%lld sum=%lld\n", e.w, e.h, e.pairs, tb_band_rows_equal(b), R, sum_steps(10, 2, e.h, e.R0), sum_steps(10, 2, e.h, R));
    }
    // 16 pairs per lane, the other levels: 864 rows -2.6 %, 691 rows -7.0 %, 553 rows -1.8 %
    const struct { int w, h; double gain; } ex16[] = {{1536, 864, 0.026}, {1229, 691, 0.070}, {983, 553, 0.018}};
    for (const auto &e : ex16) {
        const TbBandShape b{10, 2, e.h, jw_per_band(e.w, 16), 3072, 0, 3};
        const double g = 1.0 - (double)sum_steps(10, 2, e.h, tb_band_rows(b)) / (double)sum_steps(10, 2, e.h, tb_band_rows_equal(b));
        CHECK(g > e.gain - 0.002 && g < e.gain + 0.002);
        if (fails) std::printf("  16 pairs %dx%d: gain %.4f\n", e.w, e.h, g);
    }
    if (fails) { std::printf("tvl1_band_test: FAILED\n"); return 1; }
    std::printf("tvl1_band_test: ok\n");
    return 0;
}
