// fcnet_plan_check.cpp -- what the fcnet kernels rely on without saying so, checked on every shape dcomp_actor_create accepts.
// A stand-alone host program: it includes the plan header (deepcomp_amd/csrc/dcomp_fcnet_plan.h) and nothing of HIP.
// tests/test_fcnet_matrix_cpu.py compiles it with -fsanitize=address,undefined and expects exit status 0.
#include <cstdio>
#include <cstdlib>

#include "../deepcomp_amd/csrc/dcomp_fcnet_plan.h"

using namespace dlearn;
using namespace dplan;

static long long failures = 0;

#define CHECK(cond, ...)                                    \
    do {                                                    \
        if (!(cond)) {                                      \
            if (failures++ < 20) {                          \
                std::printf("FAILED %s at ", #cond);        \
                std::printf(__VA_ARGS__);                   \
                std::printf("\n");                          \
            }                                               \
        }                                                   \
    } while (0)

static void check_shape(int kind, int U, int B, int H)
{
    const ActorPlan a = actor_plan(kind, U, B, H);
#define AT "kind %d U %d B %d H %d", kind, U, B, H
    CHECK(a.K1p % 16 == 0 && a.K1 <= a.K1p && a.K1p < a.K1 + 16, AT);                  // layer1 walks whole k steps of 16
    CHECK(32 * a.NT3 >= a.N3 && a.N3 > 32 * (a.NT3 - 1), AT);
    CHECK(a.NT3v == (a.N3 % 32 == 0 ? a.NT3 + 1 : a.NT3), AT);                        // the value's column: a tile of its own exactly then
    CHECK(a.XS * 2 % 16 == 0 && (a.XS * 2 / 16) % 2 == 1, AT);                        // 16-byte fragment reads, conflict-free rows
    CHECK(a.lds_per_wave * WAVES <= 65536, AT);
    CHECK(a.chunks * KC >= a.K1p && a.K1p > (a.chunks - 1) * KC, AT);
    CHECK(a.Hp == 32 * a.mt && a.KS2 == 2 * a.mt && a.Hp >= H && (a.mt == 1 || a.mt == 2 || a.mt == 4 || a.mt == 8), AT);
    const LearnerPlan l = learner_plan(a);
    int ntask = 0;
    for (int i = 0; i < 6; i++) {
        CHECK(l.in_p[i] % 32 == 0 && l.out_p[i] % 32 == 0, AT);
        const int mi = l.in_p[i] / 32, ni = l.out_p[i] / 32;
        CHECK(l.mb[i] >= 1 && l.nb[i] >= 1 && mi % l.mb[i] == 0 && ni % l.nb[i] == 0, AT);
        CHECK(l.first_task[i] == ntask && l.nmain[i] == (mi / l.mb[i]) * (ni / l.nb[i]), AT);
        ntask += l.nmain[i] + ni / l.nb[i];
    }
    CHECK(l.ntask == ntask, AT);
    CHECK(l.K1pp % 32 == 0 && l.K1pp >= a.K1 && l.N3p >= a.N3, AT);
    long long total = 0;
    for (int i = 0; i < NARR; i++) {
        CHECK(l.off[i] == total && l.len[i] == l.nin[i] * l.nout[i] && l.len[i] > 0, AT);
        total += l.len[i];
    }
    CHECK(total == l.total && total <= 0x7FFFFFFFll, AT);
#undef AT
}

int main()
{
    long long shapes = 0;
    const int kinds[2] = {DCOMP_CENTRAL, DCOMP_MULTI};
    for (int kind : kinds)
        for (int U = 1; U <= DCOMP_MAX_UE; U++)
            for (int B = 1; B <= DCOMP_MAX_BS; B++) {
                const ActorPlan a = actor_plan(kind, U, B, 32);
                if (a.K1 > DCOMP_ACTOR_MAX_IN || a.N3 > DCOMP_ACTOR_MAX_LOGITS) continue;        // (dcomp_actor_create refuses it)
                for (int H = 32; H <= DCOMP_ACTOR_MAX_HIDDEN; H += 32, shapes++) check_shape(kind, U, B, H);
            }
    const long long rows[] = {1, 31, 32, 33, 2048ll * 128 - 1, 2048ll * 128, 2048ll * 128 + 1, 264250, 1ll << 28};
    for (long long r : rows) {
        const RowSplit s = row_split(r);
        CHECK(s.tiles * TILE == s.rows_pad && s.rows_pad >= r && s.rows_pad < r + TILE, "rows %lld", r);
        CHECK(s.nchunks >= 1 && s.nchunks <= MAX_CHUNKS, "rows %lld", r);               // the partials are [MAX_CHUNKS][in_p][out_p]
        CHECK(s.chunk_rows % CHUNK_UNIT == 0 && s.chunk_rows == CHUNK_UNIT * s.mult, "rows %lld", r);
        CHECK((long long)s.nchunks * s.chunk_rows >= s.rows_pad, "rows %lld", r);
        CHECK(LearnerPlan::ld_of(r) % 32 == 0 && LearnerPlan::ld_of(r) >= s.rows_pad, "rows %lld", r);
    }
    CHECK(max_blocks_of(0) == 512 && max_blocks_of(256) == 512 && launch_blocks(1, 512) == 1 && launch_blocks(5, 512) == 2 && launch_blocks(1 << 20, 512) == 512, "the grid");
    std::printf("%lld shapes, %d row counts, %lld failures\n", shapes, (int)(sizeof(rows) / sizeof(rows[0])), failures);
    return failures ? 1 : 0;
}
