// What the host halves of the feature units share (api_eval.hip's nearest part, api_info.hip, api_hac.hip, api_kmeans.hip,
// api_motion.hip, api_mfcc.hip; included behind ctx.hip.h): how a refusal is worded, how a caller's workspace is cut up, who owns the device
// memory of a host-array wrapper, and the pick of a kernel's element type.  No policy lives here: which checks an entry point
// makes, in which order, and what its workspace holds stay with its unit.
#pragma once

namespace klnmf_host {

constexpr int64_t kMaxInt = 0x7fffffffLL;           // 2^31 - 1: what a count, an index or a grid of the feature kernels stays below

inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// The refusals of the entry point `who`: fail() with "<who>: <what>".  An entry point makes all of them before it touches anything.
struct Who {
    const char *who;
    [[noreturn]] void bad(const std::string &what) const { fail(KLNMF_ERR_ARG, std::string(who) + ": " + what); }
    [[noreturn]] void unsupp(const std::string &what) const { fail(KLNMF_ERR_UNSUPP, std::string(who) + ": " + what); }
    void dtype(int dt, const char *prefix = "") const {          // prefix: "value_" for an argument called value_dtype
        if (dt != KLNMF_DT_F32 && dt != KLNMF_DT_F64) bad(std::string(prefix) + kDtypeMsg);
    }
    void workspace(uint64_t work_bytes, size_t need, const char *sizer) const {
        if (work_bytes < (uint64_t)need) bad(std::string("workspace below ") + sizer);
    }
};

// A caller's workspace as a running byte offset: take() returns where a piece starts and moves on by its size rounded up to 16.
// Alternatives that share the front of the buffer (one call at a time uses it) are laid out each on its own from 0 and overlaid.
struct WorkLayout {
    size_t end = 0;
    size_t take(size_t bytes) {
        const size_t at = end;
        end += up16(bytes);
        return at;
    }
    void overlay(std::initializer_list<WorkLayout> alts) { for (const WorkLayout &a : alts) end = std::max(end, a.end); }
};

// The device memory of a host-array wrapper: freed when the wrapper returns or a refusal unwinds it.
struct DeviceScratch {
    std::vector<void *> held;
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch &) = delete;
    DeviceScratch &operator=(const DeviceScratch &) = delete;
    ~DeviceScratch() { for (void *p : held) (void)hipFree(p); }
    void *take(size_t bytes) {
        held.reserve(held.size() + 1);
        void *p = nullptr;
        HIPCHK(hipMalloc(&p, std::max<size_t>(bytes, 16)));
        held.push_back(p);
        return p;
    }
};

// f(TypeTag<double>{}) or f(TypeTag<float>{}) by a KLNMF_DT_* that has passed Who::dtype.
template <typename F>
void by_dtype(int dtype, F &&f) {
    dispatch_type(dtype == KLNMF_DT_F64, f);
}

inline size_t dtype_bytes(int dtype) { return dtype == KLNMF_DT_F64 ? 8 : 4; }

}  // namespace klnmf_host
