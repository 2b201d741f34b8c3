// The inner keys of the random stream (pathed_amd/csrc/shading.h: innerKey, fillKeyRow, drawFromRow, RowRng, KeySlots) on the
// host: the very text k_path_small_single runs, against Rng::next().  Stand-alone, no device code, no HIP call:
//   hipcc --cuda-host-only -std=c++17 -O1 -Iinclude -iquote pathed_amd/csrc tests/key_rows_host.hip -o key_rows_host
//   key_rows_host <random cases>
// (tests/test_key_rows_host.py builds it plain and with -fsanitize=address,undefined)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "pathed_hip.h"
#include "shading.h"

using namespace pathed;

static int failures = 0;
#define EXPECT(condition)                                                                  \
    do {                                                                                   \
        if (!(condition)) {                                                                \
            if (failures++ < 20) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #condition); } \
        }                                                                                  \
    } while (0)

static uint32_t bitsOf(float value)
{
    uint32_t bits;
    std::memcpy(&bits, &value, sizeof bits);
    return bits;
}

// one draw: column j of the row of (k1, vertex) against Rng::next() at dimension vertexBase(vertex) + j
static void checkDraw(uint32_t k0, uint32_t k1, int vertex, int column)
{
    uint32_t row[kKeyRowWords];
    fillKeyRow(k1, vertex, row);
    Rng random;
    random.k0 = k0; random.k1 = k1; random.dimension = vertexBase(vertex) + (uint32_t)column;
    const float expected = random.next();
    EXPECT(bitsOf(drawFromRow(k0, row, (uint32_t)column)) == bitsOf(expected));
    EXPECT(row[column] == innerKey(k1, vertexBase(vertex) + (uint32_t)column));
}

// the numbers of a whole vertex in the order pathDepart draws them: the BSDF's from column 0, the light's from column 3
static void checkVertex(uint32_t k0, uint32_t k1, int vertex)
{
    uint32_t row[kKeyRowWords];
    fillKeyRow(k1, vertex, row);
    Rng random;
    random.k0 = k0; random.k1 = k1;
    RowRng rowRandom;
    rowRandom.k0 = k0; rowRandom.row = row;
    const uint32_t starts[2] = { 0u, 3u };
    const int counts[2] = { 3, 5 };   // (as many as the row holds from there)
    for (int part = 0; part < 2; part++) {
        random.dimension = vertexBase(vertex) + starts[part];
        rowRandom.dimension = starts[part];
        for (int k = 0; k < counts[part]; k++) {
            const float expected = random.next();
            EXPECT(bitsOf(rowRandom.next()) == bitsOf(expected));
        }
        EXPECT(rowRandom.dimension == starts[part] + (uint32_t)counts[part]);
        EXPECT(random.dimension == vertexBase(vertex) + rowRandom.dimension);
    }
}

// A wave's table as the kernel lays it out: kKeyVertices rows from vertex 1 on, word w keys dimension vertexBase(1) + w.
static void checkTable(uint32_t k1)
{
    std::vector<uint32_t> table(kKeyTableWords);
    for (int w = 0; w < kKeyTableWords; w++) { table[w] = innerKey(k1, vertexBase(1) + (uint32_t)w); }
    for (int vertex = 1; vertex <= kKeyVertices; vertex++) {
        uint32_t row[kKeyRowWords];
        fillKeyRow(k1, vertex, row);
        EXPECT(std::memcmp(row, table.data() + (vertex - 1) * kKeyRowWords, sizeof row) == 0);
    }
}

static void checkSlots()
{
    KeySlots slots;
    slots.clear();
    EXPECT(slots.find(0u) == -1 && slots.find(7u) == -1);   // empty tables hold no key, not even 0
    EXPECT(slots.claim(0u) == 0);                           // miss: the first empty table
    EXPECT(slots.find(0u) == 0 && slots.find(7u) == -1);    // hit, miss
    EXPECT(slots.claim(7u) == 1);                           // the second empty table
    EXPECT(slots.find(0u) == 0 && slots.find(7u) == 1);
    EXPECT(slots.claim(9u) == 0);                           // evict: the older table, 0's
    EXPECT(slots.find(0u) == -1 && slots.find(7u) == 1 && slots.find(9u) == 0);
    EXPECT(slots.claim(11u) == 1);                          // ... then 7's
    EXPECT(slots.find(7u) == -1 && slots.find(9u) == 0 && slots.find(11u) == 1);
    EXPECT(slots.claim(7u) == 0);                           // re-use: a key that was evicted comes back into the older table
    EXPECT(slots.find(7u) == 0 && slots.find(11u) == 1 && slots.find(9u) == -1);
    EXPECT(slots.claim(0xFFFFFFFFu) == 1);
    EXPECT(slots.find(0xFFFFFFFFu) == 1 && slots.find(7u) == 0 && slots.find(11u) == -1);
    // a scripted run against a model that remembers the order of claims
    std::mt19937 generator(3);
    uint32_t held[2] = { 7u, 0xFFFFFFFFu };   // table -> key
    int older = 0;
    for (int step = 0; step < 10000; step++) {
        const uint32_t k1 = generator() % 5u;
        const int expected = held[0] == k1 ? 0 : held[1] == k1 ? 1 : -1;
        EXPECT(slots.find(k1) == expected);
        if (expected < 0) {
            EXPECT(slots.claim(k1) == older);
            held[older] = k1;
            older ^= 1;
        }
    }
}

int main(int argc, char **argv)
{
    const long cases = argc > 1 ? std::atol(argv[1]) : 1000000;
    std::mt19937 generator(1);
    for (long i = 0; i < cases; i++) {
        const uint32_t k0 = generator(), k1 = generator();
        const int vertex = 1 + (int)(generator() % 40u);   // beyond the tables too: such a lane fills its own row
        checkDraw(k0, k1, vertex, (int)(generator() % (uint32_t)kKeyRowWords));
    }
    // the corners: all-zero and all-one keys, the first and the last vertex of a table, and the vertices around which the
    // dimension's product with the stride and the dimension itself wrap (vertexBase(2^29 + 1) = 2 + 2^32 = 2)
    const uint32_t corners[] = { 0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0x9e3779b9u, 0x61c88647u };
    const int vertices[] = { 1, 2, kKeyVertices, kKeyVertices + 1, 15, 0x0FFFFFFF, 0x10000000, 0x1FFFFFFF, 0x20000000, 0x20000001, 0x7FFFFFFF };
    for (uint32_t k0 : corners) {
        for (uint32_t k1 : corners) {
            for (int vertex : vertices) {
                for (int column = 0; column < kKeyRowWords; column++) { checkDraw(k0, k1, vertex, column); }
                checkVertex(k0, k1, vertex);
            }
            checkTable(k1);
        }
    }
    for (int i = 0; i < 1000; i++) { checkVertex(generator(), generator(), 1 + (int)(generator() % 16u)); }
    checkSlots();
    std::printf("key rows: %ld random draws, %d failures\n", cases, failures);
    return failures == 0 ? 0 : 1;
}
