/*
 * osmt_pool_layout.h — where the arrays of one device allocation go.  Host only, no HIP: tests/pool_layout_shim.cpp
 * builds it with g++.
 *
 * Every array starts on a 256-byte boundary, and an empty array still takes 4 bytes: it gets an offset of its own, so a
 * pointer formed from it is a valid device address that no neighbour shares (a kernel handed count 0 never reads it, a
 * hipMemset of "count + 1" words over it stays inside the allocation).
 */
#ifndef OSMT_POOL_LAYOUT_H
#define OSMT_POOL_LAYOUT_H

#include <cstddef>

namespace osmt_host {

constexpr size_t POOL_ALIGN = 256, POOL_MIN_BYTES = 4;

class pool_layout {
   public:
    /* the offset of an array of `bytes` bytes behind everything added so far */
    size_t add(size_t bytes) {
        const size_t o = total_;
        total_ = (o + (bytes < POOL_MIN_BYTES ? POOL_MIN_BYTES : bytes) + POOL_ALIGN - 1) / POOL_ALIGN * POOL_ALIGN;
        return o;
    }
    /* what the allocation takes: a multiple of 256 */
    size_t size() const { return total_; }

   private:
    size_t total_ = 0;
};

}  // namespace osmt_host

#endif
