// bp_r1cs_batch_verify_locate: which proofs of a failing batch are the bad ones.  This file is the PLANNER — plain host C++, no HIP:
// it decides which subsets of the batch go through the batch verifier's core (a PASS) and reads the statuses off the outcomes.  The
// entry points (arkbp.hip) hand it the real core as its callback, bp_debug_locate_plan a simulator; both run the code below.
//
// The planner works on the list of SURVIVORS, in instance order: the instances that did not fail before their check.  A pass covers
// a contiguous range [lo, lo + n) of that list and has one of three outcomes:
//   passed        the weighted sum of the range is the identity: every member is BP_OK (batch_verify's soundness over the weights);
//   failed_check  it is not: at least one member is invalid;
//   failed_before some members failed before the check (framing, decompression, replay): the core names ALL of them at once, with
//                 their statuses, and gives no verdict on the rest.
// Rules: pass 1 covers everything; members that failed before the check leave with their statuses and the survivors are run again.
// A failed range of at most `leaf` members is decided exactly (one member: it IS the failure — alpha * C is the identity iff C is,
// alpha != 0; more: the caller's exact per-instance verifier).  A larger failed range is halved, lower half floor(n / 2): the lower
// half is tested; when it passes, the upper half is known to fail and is split WITHOUT a pass of its own; when it fails, it is
// searched and the upper half tested after it.  With f >= 1 invalid members among n survivors and leaf = 1 that is at most
// 1 + 2 f ceil(log2 n) passes (either half holds at most ceil(n / 2) members); a valid batch is one pass.  For f = 1 the passes
// cover at most 3 n instances in all: beyond pass 1 a range of n costs S(n) <= 2 n - 2, by induction over
// S(n) = max(n + S(floor(n / 2)), floor(n / 2) + S(ceil(n / 2))) — the bad member in the lower half costs both halves' passes, in
// the upper half only the lower one's.  The SMALLER half has to be the tested one for that: with the lower half ceil(n / 2) the
// first member of n = 2^k + 1 costs n + S(ceil(n / 2)), 28 > 27 instances at n = 9.
#include <cstdint>
#include <functional>
#include <utility>
#include <vector>

struct LocateOutcome {
    enum Kind { PASSED = 0, FAILED_CHECK = 1, FAILED_BEFORE = 2 };
    Kind kind = PASSED;
    std::vector<std::pair<size_t, int>> before;   // FAILED_BEFORE: (position in the range, status), ascending
};

class LocatePlanner {
public:
    // run(lo, n, out): one pass over survivors()[lo .. lo + n); non-zero = the pass could not run (the plan stops with that code)
    typedef std::function<int(size_t, size_t, LocateOutcome&)> RunFn;
    // exact(lo, n, st): st[j] = the exact status of survivors()[lo + j], each on its own; non-zero = could not run
    typedef std::function<int(size_t, size_t, int*)> ExactFn;

    LocatePlanner(size_t count, size_t leaf, int* status) : leaf_(leaf ? leaf : 1), status_(status) {
        surv_.resize(count);
        for (size_t k = 0; k < count; k++) { surv_[k] = (uint32_t)k; status_[k] = 0; }
    }
    const std::vector<uint32_t>& survivors() const { return surv_; }
    uint64_t passes() const { return passes_; }
    uint64_t instances_in_passes() const { return instances_; }
    uint64_t exact_leaves() const { return exact_; }

    int plan(const RunFn& run, const ExactFn& exact, int verification_code) {
        run_ = &run; exact_fn_ = &exact; vcode_ = verification_code;
        for (;;) {   // members that fail before their check leave; then the survivors as a whole
            if (surv_.empty()) return 0;
            LocateOutcome out;
            const int rc = pass(0, surv_.size(), out);
            if (rc) return rc;
            if (out.kind == LocateOutcome::PASSED) return 0;   // (statuses are 0 already)
            if (out.kind == LocateOutcome::FAILED_CHECK) break;
            if (out.before.empty()) return -1;   // (BP_E_ARG: a core that names nobody would not let the plan advance)
            std::vector<uint32_t> keep;
            size_t at = 0;
            for (size_t j = 0; j < surv_.size(); j++) {
                if (at < out.before.size() && out.before[at].first == j) { status_[surv_[j]] = out.before[at].second; at++; }
                else keep.push_back(surv_[j]);
            }
            surv_.swap(keep);
        }
        return search(0, surv_.size());
    }

private:
    int pass(size_t lo, size_t n, LocateOutcome& out) {
        passes_++; instances_ += n;
        return (*run_)(lo, n, out);
    }
    int decide(size_t lo, size_t n) {   // a range that fails its check and is not split further
        exact_ += n;
        if (n == 1) { status_[surv_[lo]] = vcode_; return 0; }
        std::vector<int> st(n, 0);
        const int rc = (*exact_fn_)(lo, n, st.data());
        if (rc) return rc;
        for (size_t j = 0; j < n; j++) status_[surv_[lo + j]] = st[j];
        return 0;
    }
    // a range after its own pass.  Members that fail before the check cannot appear here (pass 1 saw every instance from the same
    // entry state); if a core reports some all the same, the range is decided exactly and nothing is implied about its sibling.
    enum Tested { T_PASSED, T_FAILED, T_DECIDED };
    int test(size_t lo, size_t n, Tested& res) {
        LocateOutcome out;
        const int rc = pass(lo, n, out);
        if (rc) return rc;
        res = out.kind == LocateOutcome::PASSED ? T_PASSED : T_FAILED;
        if (out.kind != LocateOutcome::FAILED_BEFORE) return 0;
        res = T_DECIDED;
        exact_ += n;
        std::vector<int> st(n, 0);
        const int erc = (*exact_fn_)(lo, n, st.data());
        if (erc) return erc;
        for (size_t j = 0; j < n; j++) status_[surv_[lo + j]] = st[j];
        return 0;
    }
    int search(size_t lo, size_t n) {   // [lo, lo + n) is known to fail its check
        if (n <= leaf_) return decide(lo, n);
        const size_t h = n / 2;   // (n >= 2 here)
        Tested lower = T_PASSED, upper = T_PASSED;
        int rc = test(lo, h, lower);
        if (rc) return rc;
        if (lower == T_PASSED) return search(lo + h, n - h);   // implied: the upper half fails, no pass of its own
        if (lower == T_FAILED) { rc = search(lo, h); if (rc) return rc; }
        rc = test(lo + h, n - h, upper);
        if (rc) return rc;
        return upper == T_FAILED ? search(lo + h, n - h) : 0;
    }

    size_t leaf_;
    int* status_;
    int vcode_ = 0;
    const RunFn* run_ = nullptr;
    const ExactFn* exact_fn_ = nullptr;
    std::vector<uint32_t> surv_;
    uint64_t passes_ = 0, instances_ = 0, exact_ = 0;
};
