// scratch.h -- a slice of a handle's workspace as a plain value: what the GEMMs and column sums need of a handle (where their
// split-K slabs / partials may lie, how many bytes, how many CUs to fill) and nothing else of it.  Host-only and free of HIP
// (tests/host/lstm_forms_check.cpp).
#pragma once
#include <stddef.h>

struct uav_scratch {
    char* p;
    size_t bytes;
    int num_cu;

    // The one carving operation: take `n` bytes off the tail, with at least `front` bytes left in front of them for whoever
    // gets the rest.  *tail = where the n bytes lie (p + bytes - n, no rounding: the callers' sizes are whole floats or
    // already rounded); returns the slice in front of them.  When n + front exceeds the slice, nothing is carved: *tail
    // = NULL and the returned slice has p == NULL, for the caller's UAV_REQUIRE.  carve(0, 0, ..) returns the slice as it is.
    template <class T>
    uav_scratch carve(size_t n, size_t front, T** tail) const {
        if (n > bytes || front > bytes - n) {
            *tail = nullptr;
            return uav_scratch{nullptr, 0, num_cu};
        }
        *tail = reinterpret_cast<T*>(p + (bytes - n));
        return uav_scratch{p, bytes - n, num_cu};
    }
};
