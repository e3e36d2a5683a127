// rtdm_rows.h -- THE host copy of pitched rows between a caller's plane and a handle's page-locked staging: every host entry
// point of the C ABI layer moves its rows with copy_rows.  Plain C++11, no HIP: tests/rows_host.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstring>

namespace rtdm {

// Whose bytes lie between row_bytes and the pitch of a destination row: KEEP the caller's (a view into a larger plane; exactly
// row_bytes per row are written), OURS the handle's staging (they may take whatever the source holds there).
enum class RowPad { KEEP, OURS };

// `rows` rows of row_bytes bytes, from rows src_pitch apart to rows dst_pitch apart.  Rows that lie alike on both sides move as
// one memcpy: with KEEP only where they carry no pad at all, with OURS wherever the pitches are equal.  In both modes nothing
// is read or written behind row_bytes of the last row: a view that starts at x > 0 of its parent plane ends before the row's
// pitch does.  A row range [y0, y1) is the caller's to express by offsetting both pointers.
inline void copy_rows(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t row_bytes, int rows, RowPad dst_pad)
{
    if (rows <= 0 || row_bytes == 0) return;
    if (dst_pitch == src_pitch && (dst_pad == RowPad::OURS || dst_pitch == row_bytes)) {
        memcpy(dst, src, (size_t)(rows - 1) * dst_pitch + row_bytes);
        return;
    }
    for (int y = 0; y < rows; ++y)
        memcpy((unsigned char*)dst + (size_t)y * dst_pitch, (const unsigned char*)src + (size_t)y * src_pitch, row_bytes);
}

}  // namespace rtdm
