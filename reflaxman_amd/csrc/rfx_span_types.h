// Parameter record and launches of the span queries (include/rfx.h "Ray intervals": rfx_query_hits_span,
// rfx_query_occluded_span and their ordered forms), shared by the host unit (rfx_span.cpp) and the device unit
// (rfx_trace_span.hip).  Declarations only.
#pragma once
#include <hip/hip_runtime.h>

#include "rfx_types.h"

namespace rfx {

// One launch of a span query: a hit query's record (H) and the interval arrays.  Linear and raster launches (order
// null): rays [0, H.n) of every pointer, each starting at the launch's first ray.  Ordered launches: the slots
// [slot0, slot1) of `order`, each naming a ray of the whole batch (H.n rays, H.W unused); the interval arrays are
// indexed by the ray, as H's are.
struct SpanParams {
  HitParams H;
  const float *lo;        // per ray, or null: no lower end
  const int32_t *after;   // per ray, or null: -1; read only where lo is given (closest hit only)
  const float *hi;        // per ray, or null: no upper end
  const uint32_t *order;
  uint64_t slot0, slot1;
};

// ---- rfx_trace_span.hip: one launch of a span query -- any: the any-hit kernel, else the closest-hit one; P.order
// chooses the ordered kernels
hipError_t launch_query_span(const DevScene &S, const SpanParams &P, bool any, hipStream_t st);

}  // namespace rfx
