// The chunk arithmetic of the staged host uploads, as pure functions: no HIP, no context (tests/stage_chunks_check.cpp walks it on
// the host alone).  A host block [rows, cols] whose rows lie `ld` elements of `es` bytes apart crosses the bus through one device
// staging buffer of at most about kStageBytes, `rows_per` rows per chunk; a chunk's copy ends with its last row's `cols` elements,
// so it never reads past the block's own ((rows - 1) * ld + cols) * es bytes.  Used by staged_upload (ctx.hip.h), the one loop
// behind klnmf_upload_V / _weights / _presence and klnmf_batch_upload_V / _presence.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace klnmf_host {

constexpr size_t kStageBytes = 256ull << 20;

// rows per chunk: what fits the bound, at least 1 (a single row may be longer than the bound), at most `rows`
inline int64_t stage_rows_per(int64_t rows, int64_t ld, size_t es) {
    const int64_t fit = (int64_t)(kStageBytes / std::max<size_t>(1, es * (size_t)ld));
    return std::min(rows, std::max<int64_t>(1, fit));
}
// the staging buffer (the 16: a block without rows or columns still gets an allocation)
inline size_t stage_alloc_bytes(int64_t rows_per, int64_t ld, size_t es) { return (size_t)rows_per * ld * es + 16; }

struct StageChunk {
    int64_t r0, rr;           // the chunk's first row and its row count
    size_t offset, bytes;     // its copy: `bytes` from `offset` of the host block
};
// f(chunk) for every chunk, in order
template <typename F>
void stage_walk(int64_t rows, int64_t cols, int64_t ld, size_t es, int64_t rows_per, F &&f) {
    for (int64_t r0 = 0; r0 < rows; r0 += rows_per) {
        const int64_t rr = std::min(rows_per, rows - r0);
        f(StageChunk{r0, rr, (size_t)r0 * ld * es, ((size_t)(rr - 1) * ld + cols) * es});
    }
}

}  // namespace klnmf_host
