// sp_carve.h -- plain C++ (no HIP types): the host compiler alone can run a layout on a null base (tests/c2plan_host_check.cpp)
#pragma once
#include <stddef.h>
#include <stdint.h>

// bump carver: arrays laid out one after the other in a device buffer, each at a 256-byte-aligned offset.  A layout is
// a function of the carver that makes its take() calls in buffer order: run on sp_carve() it sizes the buffer (`off`),
// run on sp_carve(buffer) it hands out the pointers.
struct sp_carve {
    uintptr_t base;
    size_t off = 0;
    explicit sp_carve(void *buffer = nullptr) : base((uintptr_t)buffer) {}
    template <typename T>
    T *take(size_t n) {
        T *p = (T *)(base + off);
        off += (n * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
};
