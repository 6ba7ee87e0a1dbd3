// ragged_reads.hpp -- the argument check every entry point that takes ragged
// reads makes of them: read i is seqs[offsets[i] .. offsets[i] + lengths[i]).
// Header-only host C++, no HIP.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

namespace ldpc {
namespace ragged {

// The extent of n reads: *total = the bytes of seqs they span, *max_len (may be
// null) the longest.  A zero-length read spans nothing wherever its offset
// points, unless count_empty (ldpc_dna_edit_distance uploads up to it).
// Returns the message of a bad entry, or an empty string.
inline std::string extent(const int64_t* offsets, const int32_t* lengths, int64_t n, int64_t* total,
                          bool count_empty = false, int32_t* max_len = nullptr)
{
    *total = 0;
    if (max_len) *max_len = 0;
    for (int64_t i = 0; i < n; i++) {
        if (lengths[i] < 0 || offsets[i] < 0 || offsets[i] > INT64_MAX - lengths[i])
            return "negative or overflowing length/offset";
        if (lengths[i] > 0 || count_empty) *total = std::max<int64_t>(*total, offsets[i] + lengths[i]);
        if (max_len) *max_len = std::max(*max_len, lengths[i]);
    }
    return std::string();
}

// extent(), and seqs may be null only when the reads span no byte.
inline std::string check(const uint8_t* seqs, const int64_t* offsets, const int32_t* lengths, int64_t n, int64_t* total)
{
    std::string err = extent(offsets, lengths, n, total);
    if (err.empty() && *total > 0 && !seqs) err = "null sequences";
    return err;
}

}  // namespace ragged
}  // namespace ldpc
