// rua_wave.h — wave and workgroup geometry of gfx950, for device code and host-only code alike.
#pragma once
#define RUA_WAVE 64          // gfx950 wavefront
#define RUA_BLOCK 256        // 4 waves per workgroup everywhere
#define RUA_WAVES_PER_BLOCK (RUA_BLOCK / RUA_WAVE)
