// A ragged batch on the host side of the C ABI: pairs of different sizes in slots padded to Np x Mp (include/mdgat_hip.h, "Ragged
// batches"), described once, and the one function that checks the description before anything is launched.
#pragma once
#include <stddef.h>

// The pairs' own keypoint counts, twice: device int32 [B] for the kernels, the same values on the host for mdgat_check_ragged.
struct RaggedCounts {
    const int *cnt0 = nullptr, *cnt1 = nullptr, *host0 = nullptr, *host1 = nullptr;
    explicit operator bool() const { return cnt0 != nullptr; }
    // the same from pair c on
    RaggedCounts from(size_t c) const {
        auto o = [c](const int* q) { return q ? q + c : q; };
        return RaggedCounts{o(cnt0), o(cnt1), o(host0), o(host1)};
    }
};

// A ragged chunk out of a bank of records [rows0 | rows1][37]: frame f of pair b is the counts[b] records from row start[b] - device
// int64 [B] for the kernel that reads the records (the exact mode's assemble kernel, the fp32-class encoder's bank form), host copies for
// the check.
struct RaggedStarts {
    const long long *start0 = nullptr, *start1 = nullptr, *host0 = nullptr, *host1 = nullptr;
    long long rows0 = 0, rows1 = 0;
    explicit operator bool() const { return start0 != nullptr; }
    RaggedStarts from(size_t c) const {
        auto o = [c](const long long* q) { return q ? q + c : q; };
        return RaggedStarts{o(start0), o(start1), o(host0), o(host1), rows0, rows1};
    }
};

// Every per-pair check of a ragged batch, on the host copies, for entry `who` (api.hip).  First the count vectors, and with a bank its
// start vectors, must not be null ("<who>: null counts pointer" / "null starts pointer").  Then pair by pair, the first offending pair
// named by its index:
//   1 <= counts0[b] <= Np and 1 <= counts1[b] <= Mp;
//   no k of the schedule topk[0 .. ntopk) exceeds min(counts0[b], counts1[b]), the keys of the pair's smaller frame (torch.topk raises
//   in the reference, mdgat.py:202; ntopk = 0: no schedule; with more than one entry the refusal names the layer);
//   with a bank, the records start[b] .. start[b] + counts[b] lie inside its rows.
// MDGAT_ERR_BAD_ARG for each; *cnt_min (optional) receives the smallest count of any frame (min(Np, Mp) for B = 0).
int mdgat_check_ragged(const char* who, int B, int Np, int Mp, const RaggedCounts& counts, const RaggedStarts* bank, const int* topk, int ntopk,
                       int* cnt_min);
