// rua_wave.h — wave and workgroup geometry of gfx950, for device code and host-only code alike.
#pragma once
#include <stdint.h>
#define RUA_WAVE 64          // gfx950 wavefront
#define RUA_BLOCK 256        // 4 waves per workgroup everywhere
#define RUA_WAVES_PER_BLOCK (RUA_BLOCK / RUA_WAVE)

// log2 of the lanes a row of `lpr` lanes occupies in a wave instruction (6: the whole wave, or more than one); host code
// (the reducers' and the row mover's plans)
inline int lanes_log2(int64_t lpr) {
  int lp_log2 = 0;
  while ((1 << lp_log2) < lpr && lp_log2 < 6) ++lp_log2;
  return lp_log2;
}
