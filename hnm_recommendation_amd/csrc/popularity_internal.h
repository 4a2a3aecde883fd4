// Limits shared by the popularity kernels (popularity.hip, segpop.hip).
#pragma once
#include <stddef.h>

constexpr size_t POP_TABLE_CAP = (size_t)256 << 20;  // count-table bytes per slab pass
constexpr int POP_MAX_DAYS = 65536;
constexpr int POP_FILL_BLOCKS = 2048;
constexpr int POP_CHUNK_MAX = 8192;  // bits of the LDS rank bitmap (1 KiB per workgroup)
