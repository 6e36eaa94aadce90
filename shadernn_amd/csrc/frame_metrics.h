// frame_metrics.h -- the geometry of the frame-metrics kernels (frame_metrics.hip; include/snnhip.h: snnhip_frame_metrics_plan_create; DESIGN.md section
// 4.22), kept apart so that the plan, its description and the kernels agree on one statement of it.
#pragma once

namespace snnhip {

// A block of the tile kernel owns kMetricsTileH x kMetricsTileW pixels of one image: kMetricsBlocksY x kMetricsBlocksX blocks of 4x4 pixels, one per
// thread.  It also reads the block row below and the block column to the right (the halo), so that every 8x8 window anchored in the tile is complete:
// (33 * 9) / (32 * 8) = 1.16 times the tile's own bytes.  shadernn_amd/capi.py restates the tile as FRAME_METRICS_TILE; the plan's description
// carries it ("tile=32x128").
constexpr int kMetricsTileH = 32;
constexpr int kMetricsTileW = 128;
constexpr int kMetricsBlocksY = kMetricsTileH / 4;                    // 8
constexpr int kMetricsBlocksX = kMetricsTileW / 4;                    // 32
constexpr int kMetricsThreads = kMetricsBlocksY * kMetricsBlocksX;    // 256: one owned 4x4 block, and one window, per thread
constexpr int kMetricsHaloX = kMetricsBlocksX + 1;                    // 33 block columns staged
constexpr int kMetricsPositions = (kMetricsBlocksY + 1) * kMetricsHaloX; // 297 block positions staged per channel
constexpr int kMetricsFoldThreads = 256;

// what one block of the tile kernel leaves per channel, and what the fold kernel sums in index order
struct MetricsPartial {
    double ssimSum;         // sum of t over the windows anchored in the tile
    unsigned long long sse; // sum of (a - b)^2 over the tile's pixels inside the frame
};

} // namespace snnhip
