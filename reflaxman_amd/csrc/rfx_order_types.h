// Parameter records of the coherent order (include/rfx.h rfx_rays_order and the ordered calls), shared by the host
// units and the two device units that implement it (rfx_order_sort.hip, rfx_trace_ordered.hip).  Declarations only: the
// earlier device units see this header through rfx_launch.h and compile none of it.
#pragma once
#include "rfx_types.h"

namespace rfx {

// The sort's shape: a workgroup of kOrderThreads threads takes kOrderTile consecutive (key, index) pairs per digit
// pass, wave w of it the pairs [64 kOrderItems w, 64 kOrderItems (w + 1)) of the tile; digits are kOrderDigitBits wide.
constexpr uint32_t kOrderThreads = 256, kOrderWaves = kOrderThreads / 64, kOrderItems = 16;
constexpr uint32_t kOrderTile = kOrderThreads * kOrderItems;
constexpr uint32_t kOrderDigitBits = 8, kOrderDigits = 1u << kOrderDigitBits;

// The key's box (rfx.h "Coherent order"): the origin's cell on axis a is (o_a - lo[a]) * scale[a], clamped.  It rides
// in the key kernel's own arguments, not in DevScene.
struct OrderBox { float lo[3], scale[3]; };

// One launch of an ordered hit query (rfx_ordered.h): the slots [slot0, slot1) of `order`, each naming a ray of the
// whole batch H (H.n rays, H.W unused): an index >= H.n is a dead lane.
struct HitOrderParams {
  HitParams H;
  const uint32_t *order;
  uint64_t slot0, slot1;
};

}  // namespace rfx
