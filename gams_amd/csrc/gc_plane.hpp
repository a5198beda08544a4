// gc_plane.hpp -- the upload paths' fused form of gams_gc_plane (gc_plane.cpp)
#pragma once

#include <cstddef>
#include <cstdint>

// copy n bases seq -> dst and leave their ceil(n/8) plane bytes in `plane` (bits past n zero); one pass
// over the source
void gams_gc_copy_classify(uint8_t *dst, const uint8_t *seq, size_t n, uint8_t *plane);
