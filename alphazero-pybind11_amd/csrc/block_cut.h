// One allocation cut into typed arrays.  A layout is written once, as a function that takes its arrays from a BlockCut in
// order; run on a null base the same calls give the byte size of the block (every pointer null), run on the allocation they
// give the pointers.  So the size of a block and the way it is carved cannot disagree.  Plain C++: no HIP in here.
#pragma once
#include <cstddef>
#include <cstdint>

namespace azmi {

struct BlockCut {
  explicit BlockCut(void* block = nullptr) : base(static_cast<unsigned char*>(block)) {}
  // the next `count` elements of T: the offset is first raised to T's alignment (arrays in descending element size leave no padding)
  template <class T>
  T* take(size_t count) {
    off = (off + alignof(T) - 1) / alignof(T) * alignof(T);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
  unsigned char* base;
  size_t off = 0;      // bytes taken so far: behind the last take, the size of the block
};

}  // namespace azmi
