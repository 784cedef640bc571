// The chunk arithmetic of the staged host uploads (multimodal_amd/csrc/stage_chunks.h), walked on the host alone for a table of
// block shapes.  Built and run by tests/test_stage_chunks_cpu.py; exits 0 when every property holds.
#include <cstdio>
#include <cstdlib>

#include "../multimodal_amd/csrc/stage_chunks.h"

using namespace klnmf_host;

struct Case {
    const char *what;
    int64_t rows, cols, ld;
    size_t es;
};

static int failures = 0;
#define EXPECT(cond, c)                                                                                                          \
    do {                                                                                                                         \
        if (!(cond)) {                                                                                                           \
            std::printf("FAILED %s (rows=%lld cols=%lld ld=%lld es=%zu): %s\n", (c).what, (long long)(c).rows, (long long)(c).cols, \
                        (long long)(c).ld, (c).es, #cond);                                                                       \
            ++failures;                                                                                                          \
        }                                                                                                                        \
    } while (0)

int main() {
    const int64_t MiB = 1 << 20;
    const Case cases[] = {
        {"one row, cols = ld", 1, 5, 5, 4},
        {"one row, cols = 1 < ld", 1, 1, 7, 8},
        {"cols = ld, one chunk", 100, 16, 16, 8},
        {"cols = 1 < ld, one chunk", 100, 1, 16, 4},
        {"a row longer than the bound, float", 3, 10, 64 * MiB + 3, 4},            // ld * es > 256 MiB: rows_per clamps to 1
        {"a row longer than the bound, double, cols = ld", 2, 32 * MiB + 1, 32 * MiB + 1, 8},
        {"rows an exact multiple of rows_per, float", 192, 1000, MiB, 4},          // 4 MiB rows: 64 per chunk
        {"rows no multiple of rows_per, float", 200, MiB, MiB, 4},
        {"rows an exact multiple of rows_per, double", 64, 1, MiB, 8},             // 8 MiB rows: 32 per chunk
        {"rows no multiple of rows_per, double", 70, MiB - 1, MiB, 8},
        {"rows_per = rows - 1", 65, 3, MiB, 4},
        {"a row of exactly the bound", 4, 32 * MiB, 32 * MiB, 8},
    };
    for (const Case &c : cases) {
        const int64_t rows_per = stage_rows_per(c.rows, c.ld, c.es);
        EXPECT(rows_per >= 1, c);
        if (rows_per < 1) continue;      // (the walk below would not advance)
        const size_t block = ((size_t)(c.rows - 1) * c.ld + c.cols) * c.es, alloc = stage_alloc_bytes(rows_per, c.ld, c.es);
        int64_t next = 0, chunks = 0;
        stage_walk(c.rows, c.cols, c.ld, c.es, rows_per, [&](const StageChunk &ch) {
            EXPECT(ch.r0 == next, c);                                     // in order, no gap, no overlap
            EXPECT(ch.rr >= 1 && ch.rr <= rows_per, c);
            EXPECT(ch.offset == (size_t)ch.r0 * c.ld * c.es, c);          // the chunk starts at its first row
            EXPECT(ch.bytes >= ((size_t)(ch.rr - 1) * c.ld + c.cols) * c.es, c);      // ... and holds all of its rows' elements
            EXPECT(ch.offset + ch.bytes <= block, c);                     // never past the block's last element
            EXPECT(ch.bytes <= alloc, c);                                 // never past the staging buffer
            next = ch.r0 + ch.rr;
            ++chunks;
        });
        EXPECT(next == c.rows, c);                                        // [0, rows) exactly once
        EXPECT(chunks == (c.rows + rows_per - 1) / rows_per, c);
    }
    // the table itself: both clamps and both remainders are met
    EXPECT(stage_rows_per(3, 64 * MiB + 3, 4) == 1, cases[4]);
    EXPECT(stage_rows_per(192, MiB, 4) == 64 && 192 % 64 == 0, cases[6]);
    EXPECT(stage_rows_per(200, MiB, 4) == 64 && 200 % 64 != 0, cases[7]);
    EXPECT(stage_rows_per(64, MiB, 8) == 32 && stage_rows_per(70, MiB, 8) == 32, cases[8]);
    if (failures) return 1;
    std::printf("stage chunks ok: %zu cases\n", sizeof(cases) / sizeof(cases[0]));
    return 0;
}
