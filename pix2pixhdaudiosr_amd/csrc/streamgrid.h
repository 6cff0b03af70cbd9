// Grids of the grid-stride ("streaming") kernels: min(cdiv(work, 256), cap) workgroups of 256 threads that walk the rest of
// their work with the grid's stride.  Host arithmetic only.  Every launcher takes its grid from stream_grid_of() and the host
// query p2phd_stream_grid (core.hip) calls the same function, so a test that wants the loop's second trip can prove, without a
// device, that its case is past the cap -- and a changed cap makes that test fail instead of quietly running one trip.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include "common.h"

namespace p2phd {

struct StreamGrid {
  int64_t unit_work = 0;   // how much of `work` one trip of the whole grid covers
  int wanted = 0;          // workgroups without the cap
  int used = 0;            // workgroups launched (per row): used < wanted says the kernel loops
};

enum StreamFamily {
  SG_STITCH,            // segments_gather(_planar), segments_stitch(_planar): outputs per row, a quad per thread
  SG_STITCH_RAGGED,     // segments_gather_ragged, segments_stitch_ragged: outputs of the LONGEST clip row, a quad per thread; grid.y = clip rows
  SG_STITCH_STREAM,     // segments_stitch_stream: outputs per row of one window, a quad per thread; grid.y = channels
  SG_PCM,               // pcm_decode(_ex), pcm_encode(_ex): interleaved samples, one per thread
  SG_PCM_PEAK,          // pcm_peak: frames per row; four 16-byte pieces in flight per thread; rows = channels
  SG_STEREO_VEC,        // stereo_matrix, aligned rows: a quad of samples per thread
  SG_STEREO_SCALAR,     // stereo_matrix, any alignment: a sample per thread
  SG_LOUDNESS,          // loudness_blocks, loudness_short_term: a block per thread
  SG_ITEMS,             // avgpool3s2_fwd / _bwd, nhwc_to_nchw, nchw_cat_to_nhwc (16-byte pieces), nchw_to_nhwc (elements)
  SG_ACT_BWD,           // act_bwd: elements, a 16-byte piece per thread
  SG_LOSS_FWD,          // loss_fwd: padded elements P * Cp; grid sized by pieces of 8, four 16-byte pieces in flight
  SG_LOSS_BWD,          // loss_bwd: the same with the larger cap
  SG_ADAM,              // adam_step, adam_step_dev, adam_step_scaled: floats, a float4 per thread
  SG_NONFINITE,         // grads_nonfinite (inside adam_step_scaled): floats, four float4 in flight per thread
  SG_PACK_PAIR,         // timed_pack_pair: pixels, a quad per thread
  SG_SPECTRO_ENCODE,    // spectro_encode(_ex), normalisation pass: elements, one per thread
  SG_SPECTRO_STATS,     // spectro_encode(_ex), statistics of the noise rows: elements, one per thread
  SG_RANGE_VEC,         // spectro_range, range_fold, 16-byte aligned input: floats, a float4 per thread (+ a scalar tail)
  SG_RANGE_SCALAR,      // the same, any alignment: a float per thread
  SG_SPECTRO_ROWS,      // spectro_encode_rows, statistics: workgroups per row over its F * M floats, a float4 per thread; grid.y = rows
  SG_UNKNOWN
};

inline StreamFamily stream_family(const char* name) {
  static const struct { const char* name; StreamFamily f; } table[] = {
      {"segments_gather", SG_STITCH}, {"segments_gather_planar", SG_STITCH}, {"segments_stitch", SG_STITCH},
      {"segments_stitch_planar", SG_STITCH}, {"segments_gather_ragged", SG_STITCH_RAGGED}, {"segments_stitch_ragged", SG_STITCH_RAGGED},
      {"segments_stitch_stream", SG_STITCH_STREAM},
      {"pcm_decode", SG_PCM}, {"pcm_decode_ex", SG_PCM}, {"pcm_encode", SG_PCM}, {"pcm_encode_ex", SG_PCM},
      {"pcm_peak", SG_PCM_PEAK}, {"stereo_matrix", SG_STEREO_VEC}, {"stereo_matrix_scalar", SG_STEREO_SCALAR},
      {"loudness_blocks", SG_LOUDNESS}, {"loudness_short_term", SG_LOUDNESS}, {"avgpool3s2_fwd", SG_ITEMS},
      {"avgpool3s2_bwd", SG_ITEMS}, {"nchw_to_nhwc", SG_ITEMS}, {"nhwc_to_nchw", SG_ITEMS}, {"nchw_cat_to_nhwc", SG_ITEMS},
      {"act_bwd", SG_ACT_BWD}, {"loss_fwd", SG_LOSS_FWD}, {"loss_bwd", SG_LOSS_BWD}, {"adam_step", SG_ADAM},
      {"adam_step_dev", SG_ADAM}, {"adam_step_scaled", SG_ADAM}, {"grads_nonfinite", SG_NONFINITE},
      {"timed_pack_pair", SG_PACK_PAIR}, {"spectro_encode", SG_SPECTRO_ENCODE}, {"spectro_encode_ex", SG_SPECTRO_ENCODE},
      {"spectro_stats", SG_SPECTRO_STATS}, {"spectro_range", SG_RANGE_VEC}, {"range_fold", SG_RANGE_VEC},
      {"spectro_range_scalar", SG_RANGE_SCALAR}, {"range_fold_scalar", SG_RANGE_SCALAR},
      {"spectro_rows", SG_SPECTRO_ROWS}};
  for (const auto& t : table)
    if (!strcmp(name, t.name)) return t.f;
  return SG_UNKNOWN;
}

// `items` work items of one thread each, `per_trip` units of work per thread and trip
inline StreamGrid stream_capped(int64_t items, int64_t cap, int64_t per_trip) {
  StreamGrid g;
  g.wanted = (int)std::max<int64_t>(1, cdiv(items, 256));
  g.used = (int)std::min<int64_t>(g.wanted, cap);
  g.unit_work = (int64_t)g.used * 256 * per_trip;
  return g;
}

// dtype: P2PHD_F32 or P2PHD_BF16 (this library's 16-bit type), looked at where the piece of a thread depends on it.
// rows: the rows of one launch (grid.y), looked at where the cap is shared among them (SG_PCM_PEAK: channels).
inline StreamGrid stream_grid_of(StreamFamily f, int dtype, int64_t work, int rows) {
  const int epp = dtype == P2PHD_BF16 ? 8 : 4;                    // elements of a 16-byte piece
  switch (f) {
    case SG_STITCH:         return stream_capped(cdiv(work, 4), 16384, 4);
    // per clip row: a launch has up to 65535 rows of any lengths and every row gets the grid of the longest, so the cap is a row's
    // and small -- 1024 workgroups, four a CU, stream a lone long row; many short rows fill the chip by their count
    case SG_STITCH_RAGGED:  return stream_capped(cdiv(work, 4), 1024, 4);
    // per channel of a window: a window is seconds long and a file's channels few, so the cap is the ragged rows'
    case SG_STITCH_STREAM:  return stream_capped(cdiv(work, 4), 1024, 4);
    case SG_PCM:            return stream_capped(work, 16384, 1);
    case SG_PCM_PEAK: {
      // workgroups per row: enough to keep every CU busy with rows of any count, a partial table (5 words per workgroup) that
      // fits the scratch region
      const int64_t ch = std::max(rows, 1);
      const int64_t cap = std::min<int64_t>(std::max<int64_t>(1, 2048 / ch), (int64_t)(fold_capacity(FOLD_PCM).floats / (size_t)(5 * ch)));
      StreamGrid g;
      g.wanted = (int)std::max<int64_t>(1, cdiv(work / 4, 256 * 4));
      g.used = (int)std::max<int64_t>(1, std::min<int64_t>(g.wanted, cap));
      g.unit_work = (int64_t)g.used * 256 * 16;
      return g;
    }
    case SG_STEREO_VEC:     return stream_capped(cdiv(work, 4), 4096, 4);
    case SG_STEREO_SCALAR:  return stream_capped(work, 4096, 1);
    case SG_LOUDNESS:       return stream_capped(work, 2048, 1);
    case SG_ITEMS:          return stream_capped(work, 8192, 1);
    case SG_ACT_BWD:        return stream_capped(work / epp, 8192, epp);
    case SG_LOSS_FWD:       return stream_capped(work / 8, 1024, 4 * epp);
    case SG_LOSS_BWD:       return stream_capped(work / 8, 2048, 4 * epp);
    case SG_ADAM:           return stream_capped(cdiv(work, 4), 4096, 4);
    case SG_NONFINITE:      return stream_capped(cdiv(work, 4), 2048, 16);
    case SG_PACK_PAIR:      return stream_capped(cdiv(work, 4), 16384, 4);
    case SG_SPECTRO_ENCODE: return stream_capped(work, 8192, 1);
    case SG_SPECTRO_STATS:  return stream_capped(work, 1024, 1);
    case SG_RANGE_VEC:      return stream_capped(work / 4 + work % 4, 1024, 4);
    case SG_RANGE_SCALAR:   return stream_capped(work, 1024, 1);
    case SG_SPECTRO_ROWS:   return stream_capped(cdiv(work, 4), 32, 4);
    default:                return StreamGrid{};
  }
}

}  // namespace p2phd
