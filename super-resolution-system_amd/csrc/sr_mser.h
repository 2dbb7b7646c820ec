// sr_mser.h -- what sr_mser.hip (the GPU component tree) and sr_mser_host.cpp (plan, refusals, canonical order, text
// boxes, the host restatement) share.  Internal: nothing here is part of the C ABI.
#pragma once
#include <cstdint>
#include <vector>

#include "sr_internal.h"

#define MSER_MAX_PIXELS (1LL << 24)          // 4096 x 4096: int32 indices, workspace below 1 GiB (53 bytes per pixel + 12 KiB)
#define MSER_MIN_LIST_BYTES 4096             // the old-root list doubles as the record staging area of the download

// One node of the tree as the device builds it (parent: a node id of the same table, -1 for the root).
struct MserNode {
    int level, area, x0, y0, x1, y1, seed, parent;
};

// The workspace of one polarity (sections start at multiples of 256 bytes; every section is written before it is read).
struct MserPlan {
    long long npx = 0, node_cap = 0;
    size_t off_gray = 0;      // u8  [npx]       g (dark) or 255 - g (bright)
    size_t off_order = 0;     // i32 [npx]       pixel indices by level; after the tree: S per node
    size_t off_parent = 0;    // i32 [npx]       union-find parent; after the tree: indices of the kept regions
    size_t off_nor = 0;       // i32 [npx]       node id of a root (-1 none); after the tree: stable / passed bytes
    size_t off_list = 0;      // int2[npx]       (old root, its node) touched by the level; after the tree: records
    size_t off_nodes = 0;     // MserNode[npx]
    size_t off_ctr = 0;       // u32 [1024]      histogram 256, scatter cursors 256, per-level list lengths 256, node and region count
    size_t list_bytes = 0, total = 0;
};

// Every refusal of the definition (SR_ERR_UNSUPPORTED) and of the arguments (SR_ERR_INVALID_ARG); who names the caller.
int mser_check(const char *who, int h, int w, const sr_mser_params *p);
void mser_layout(int h, int w, MserPlan *out);
// Regions into the output order: polarity, level, seed.
void mser_sort_regions(sr_mser_region *r, size_t n);
// A node table in any order with parents as indices -> (level, seed) order with parent_level / parent_seed.
void mser_canonical_tree(const std::vector<MserNode> &nodes, sr_mser_node *out);
