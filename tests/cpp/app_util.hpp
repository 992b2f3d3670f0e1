// app_util.hpp -- what the test programs of this directory share: reading their binary input files, and the bit-level
// checksum of a result that the Python tests compute again (tests/cpp_apps.py, fnv1a).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mundy_hip/adapter.hpp"

/// the next `count` items of the file (an empty array reads nothing); a short file ends the program
template <class T>
inline std::vector<T> read_array(std::FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && std::fread(v.data(), sizeof(T), count, f) != count) {
    std::fprintf(stderr, "short read\n");
    std::exit(2);
  }
  return v;
}

/// What the input file of every chain step app opens with: uint64 counts[header_words] = (n, m springs, the app's own
/// counts ...), then doubles center[3n] radius[n] mob_trans[n], then int32 pairs[2m].  `file` stays open behind the
/// pairs for what the app reads next.
struct ChainInput {
  std::FILE* file;
  std::vector<std::uint64_t> counts;
  size_t n, m;
  std::vector<double> center, radius, mob_trans;
  std::vector<int32_t> pairs;
};
/// a file that does not open ends the program (status 2), as a short one does
inline ChainInput read_chain_input(const char* path, size_t header_words = 2) {
  ChainInput in;
  in.file = std::fopen(path, "rb");
  if (!in.file) {
    std::perror(path);
    std::exit(2);
  }
  in.counts = read_array<std::uint64_t>(in.file, header_words);
  in.n = in.counts[0];
  in.m = in.counts[1];
  in.center = read_array<double>(in.file, 3 * in.n);
  in.radius = read_array<double>(in.file, in.n);
  in.mob_trans = read_array<double>(in.file, in.n);
  in.pairs = read_array<int32_t>(in.file, 2 * in.m);
  return in;
}

/// order-sensitive FNV-1a over the bit patterns of a host range (items of at most 8 bytes, zero-extended)
template <class T>
inline unsigned long long fnv1a(const T* v, size_t count) {
  static_assert(sizeof(T) <= sizeof(unsigned long long), "fnv1a: items of at most 8 bytes");
  unsigned long long h = 1469598103934665603ull;
  for (size_t k = 0; k < count; ++k) {
    unsigned long long b = 0;
    std::memcpy(&b, &v[k], sizeof(T));
    h = (h ^ b) * 1099511628211ull;
  }
  return h;
}
template <class T>
inline unsigned long long checksum(const std::vector<T>& v) {
  return fnv1a(v.data(), v.size());
}
/// of the first `count` items
template <class T>
inline unsigned long long checksum(const std::vector<T>& v, size_t count) {
  return fnv1a(v.data(), count);
}
/// of `count` doubles on the device
inline unsigned long long checksum_device(const double* dev, size_t count) {
  std::vector<double> v(count);
  mundy_hip::check(mhip_memcpy_d2h(v.data(), dev, count * sizeof(double), nullptr));
  return checksum(v);
}
