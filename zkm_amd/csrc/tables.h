// tables.h -- the twelve tables of the AllStark, each described ONCE (host side): its id, its names, its profile scopes, its width, its
// own lookups and what its data-parallel writer reads.  Every module that walks "the tables" reads this registry; a thirteenth table is
// one row here, its constraint function (constraints_dev.h) and its writer (DESIGN.md "Where a table is described").
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "../../include/zkm_hip.h"

// ---- Stark::lookups(): a table's own logUp lookups
struct zkm_table_lookup { uint32_t ncols; const uint32_t* cols; uint32_t table_col, freq_col; };
// Memory: RANGE_CHECK (10) looked up in COUNTER (11) with FREQUENCIES (12), memory_stark.rs:476-483.
inline constexpr uint32_t ZKM_MEMORY_LOOKUP_COLS[1] = {10};
inline constexpr zkm_table_lookup ZKM_MEMORY_LOOKUPS[1] = {{1, ZKM_MEMORY_LOOKUP_COLS, 11, 12}};
// Arithmetic: the 18 shared columns (26..43) looked up in RANGE_COUNTER (44) with RC_FREQUENCIES (45), arithmetic_stark.rs:269-276.
inline constexpr uint32_t ZKM_ARITHMETIC_LOOKUP_COLS[18] = {26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43};
inline constexpr zkm_table_lookup ZKM_ARITHMETIC_LOOKUPS[1] = {{18, ZKM_ARITHMETIC_LOOKUP_COLS, 44, 45}};

// ---- what a data-parallel writer (witness.hip zkm_launch_writers) reads: `nlists` input lists of `k` operations, list i of
// list_bytes[i] bytes per operation, rows_per_op rows of the table per operation.  variable (the two sponges): list 0 holds the
// operations' bytes back to back (list_bytes[0] = 0) and comes with k + 1 byte offsets in host memory; the rows follow from the lengths.
// The phrases are the refusals of the table's stand-alone entry point (null: it makes no such refusal): more operations than rows, a
// null list, the flag the writer raises.  nlists = 0: no such writer (Arithmetic, Cpu and Memory have phased code of their own).
struct zkm_writer {
    uint32_t nlists;
    uint32_t list_bytes[3];
    uint32_t rows_per_op;
    bool variable;
    const char *too_many, *required, *bad;
};

struct zkm_table_row {
    int id;                     // ZKM_TABLE_*
    const char *name, *snake;   // the reference's Debug name (all_stark.rs:96-110); ours
    const char *quotient_scope, *line_scope, *writer_scope;   // profile scopes: literals, zkm_prof_scope keeps the pointer
    size_t width;
    const zkm_table_lookup* lookups;
    size_t nlookups;
    zkm_writer writer;
};

// X(ID, Debug name, snake name, lookups, their count, the writer...), in Table::all() order (all_stark.rs:117-134)
#define ZKM_TABLES(X)                                                                                                                     \
    X(ARITHMETIC, "Arithmetic", "arithmetic", ZKM_ARITHMETIC_LOOKUPS, 1, 0)                                                               \
    X(CPU, "Cpu", "cpu", nullptr, 0, 0)                                                                                                   \
    X(POSEIDON, "Poseidon", "poseidon", nullptr, 0, 2, {96, 8}, 1, false, "more permutations than 2^log_n rows",                          \
      "inputs and timestamps are required")                                                                                               \
    X(POSEIDON_SPONGE, "PoseidonSponge", "poseidon_sponge", nullptr, 0, 2, {0, 32}, 1, true)                                              \
    X(KECCAK, "Keccak", "keccak", nullptr, 0, 2, {200, 8}, 24, false, "permutations need more rows than 2^log_n (24 each)")               \
    X(KECCAK_SPONGE, "KeccakSponge", "keccak_sponge", nullptr, 0, 2, {0, 32}, 1, true)                                                    \
    X(SHA_EXTEND, "ShaExtend", "sha_extend", nullptr, 0, 2, {16, 8}, 1, false, "more rows than 2^log_n")                                  \
    X(SHA_EXTEND_SPONGE, "ShaExtendSponge", "sha_extend_sponge", nullptr, 0, 2, {64, 32}, 48, false,                                      \
      "message schedules need more rows than 2^log_n (48 each)")                                                                          \
    X(SHA_COMPRESS, "ShaCompress", "sha_compress", nullptr, 0, 3, {32, 256, 64}, 65, false, "compressions need more rows than 2^log_n")   \
    X(SHA_COMPRESS_SPONGE, "ShaCompressSponge", "sha_compress_sponge", nullptr, 0, 3, {32, 256, 64}, 1, false,                            \
      "compressions need more rows than 2^log_n")                                                                                         \
    X(LOGIC, "Logic", "logic", nullptr, 0, 1, {12}, 1, false, "more operations than 2^log_n rows", nullptr,                               \
      "op code out of range (0 and, 1 or, 2 xor, 3 nor)")                                                                                 \
    X(MEMORY, "Memory", "memory", ZKM_MEMORY_LOOKUPS, 1, 0)

#define ZKM_TABLE_ROW(ID, NAME, SNAKE, LOOKUPS, NLOOKUPS, ...) \
    {ZKM_TABLE_##ID, NAME, SNAKE, "quotient_" SNAKE, "verify/line_" SNAKE, SNAKE "_trace", ZKM_##ID##_COLS, LOOKUPS, NLOOKUPS, {__VA_ARGS__}},
inline constexpr zkm_table_row ZKM_TABLE_ROWS[] = {ZKM_TABLES(ZKM_TABLE_ROW)};
#undef ZKM_TABLE_ROW
constexpr int ZKM_NUM_TABLES = (int)(sizeof(ZKM_TABLE_ROWS) / sizeof(ZKM_TABLE_ROWS[0]));

// the row at a position of Table::all() / of a ZKM_TABLE_* id; the position of an id (-1: unknown).  Null for what is out of range.
constexpr const zkm_table_row* zkm_table_at(int enum_index) {
    return enum_index >= 0 && enum_index < ZKM_NUM_TABLES ? &ZKM_TABLE_ROWS[enum_index] : nullptr;
}
constexpr int zkm_table_index(int id) {
    for (int e = 0; e < ZKM_NUM_TABLES; e++)
        if (ZKM_TABLE_ROWS[e].id == id) return e;
    return -1;
}
constexpr const zkm_table_row* zkm_table(int id) { return zkm_table_at(zkm_table_index(id)); }

// f(std::integral_constant<int, ZKM_TABLE_X>) for the row of `id`: the one way from a run-time id to a template argument
template <class F> decltype(auto) zkm_with_table(int id, F&& f) {
    switch (id) {
#define ZKM_TABLE_CASE(ID, ...) \
    case ZKM_TABLE_##ID: return f(std::integral_constant<int, ZKM_TABLE_##ID>{});
        ZKM_TABLES(ZKM_TABLE_CASE)
#undef ZKM_TABLE_CASE
        default: throw std::runtime_error("unknown table id " + std::to_string(id));
    }
}

// the rows against an independent copy of the order: a row mistyped or moved does not compile
namespace zkm_tables_check {
constexpr int ORDER[] = {ZKM_TABLE_ARITHMETIC, ZKM_TABLE_CPU, ZKM_TABLE_POSEIDON, ZKM_TABLE_POSEIDON_SPONGE, ZKM_TABLE_KECCAK, ZKM_TABLE_KECCAK_SPONGE,
                         ZKM_TABLE_SHA_EXTEND, ZKM_TABLE_SHA_EXTEND_SPONGE, ZKM_TABLE_SHA_COMPRESS, ZKM_TABLE_SHA_COMPRESS_SPONGE, ZKM_TABLE_LOGIC,
                         ZKM_TABLE_MEMORY};
constexpr const char* NAMES[] = {"Arithmetic", "Cpu", "Poseidon", "PoseidonSponge", "Keccak", "KeccakSponge", "ShaExtend", "ShaExtendSponge",
                                 "ShaCompress", "ShaCompressSponge", "Logic", "Memory"};
constexpr bool same(const char* a, const char* b) {
    for (; *a && *a == *b; a++, b++) {}
    return *a == *b;
}
constexpr bool rows_match() {
    for (int e = 0; e < ZKM_NUM_TABLES; e++)
        if (ZKM_TABLE_ROWS[e].id != ORDER[e] || !same(ZKM_TABLE_ROWS[e].name, NAMES[e]) || !zkm_table(e) || ZKM_TABLE_ROWS[e].width == 0) return false;
    return true;
}
static_assert(ZKM_NUM_TABLES == 12 && sizeof(ORDER) / sizeof(ORDER[0]) == 12 && sizeof(NAMES) / sizeof(NAMES[0]) == 12, "twelve tables");
static_assert(rows_match(), "the rows are in Table::all() order, and their ids are a permutation of 0 .. 11");
}  // namespace zkm_tables_check
