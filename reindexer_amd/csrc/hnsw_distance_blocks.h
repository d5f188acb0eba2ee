// Which distance batch an HNSW search over rows of `dim` components takes, as a pure function: the kernel choice (hnsw_kernel_pick.h, for
// hnsw_search.hip and hnsw_server.hip), the mailbox gates (rxgpu_hnsw_server.hip) and rxgpu_hnsw_distance_blocks (include/rxgpu.h) all ask
// here.  No HIP in here — the file compiles for the host on its own.
#pragma once

#include <stdint.h>

namespace rxgpu {

// 64-float blocks (NB) of the fixed-dimension distance batch, 0: the generic batch.
//   floats: 128, 512, 768 (the whole row set in registers: batch_distances_fixed) and 1024, 1536 (in chunks: batch_distances_wide), with or
//           without deleted nodes.  384 keeps the generic batch;
//   codes:  128, 384, 512, 768, 1024, 1536 on a bare graph; the sorted-list search of a graph with deleted nodes has the fixed form for 128
//           and 768 only.
// The resident kernel serves exactly the row formats with a fixed form (hnsw_mailbox_serves).
constexpr int hnsw_distance_blocks(uint32_t dim, bool sq8, bool deleted) {
	if (sq8) {
		if (dim == 128u || dim == 768u) return int(dim / 64u);
		if (!deleted && (dim == 384u || dim == 512u || dim == 1024u || dim == 1536u)) return int(dim / 64u);
		return 0;
	}
	return (dim == 128u || dim == 512u || dim == 768u || dim == 1024u || dim == 1536u) ? int(dim / 64u) : 0;
}
constexpr bool hnsw_mailbox_serves(uint32_t dim, bool sq8, bool deleted) { return hnsw_distance_blocks(dim, sq8, deleted) != 0; }

}  // namespace rxgpu
