// CPU check of the device PNG reader's inflate: csrc/nic_inflate.h -- the very source the kernel
// compiles -- run serially over a corpus of zlib streams, meant to be built with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/png_read_host_check.cpp -o png_read_host_check
// and fed the directory tools/png_read_corpus.py writes (tests/test_png_inflate_host.py does both).
// Every corpus file is
//   u32 T (little-endian) | u8 expect (0: zlib.decompress gives exactly T bytes; 1: it raises, or the
//   length is not T) | u8 status (the exact status bits 1..8 the stream must give; 255: not pinned) |
//   u8 bytes (1: zlib's T output bytes follow) | [T bytes] | the stream
// and its buffers are heap blocks of exactly the stream's and T bytes, so an index a check let through
// is a sanitizer report.  The program fails (exit 1) when a status disagrees with `expect` or with a
// pinned `status`, when the block + symbol loop ran more than 8 * size + 1 times, when a status-0
// output differs in its Adler-32 from the stream's field (then the status carries bit 8, which
// `expect` 0 forbids), or when the output differs from zlib's bytes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../neural_network_image_compression_amd/csrc/nic_inflate.h"

namespace inf = nic::inflate;

struct HostEnv {
  const uint8_t* in;
  uint32_t size;
  uint8_t* out;
  uint32_t T;
  long calls = 0;
  int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() const {}
  uint32_t in_byte(uint32_t pos) { return in[pos]; }  // no clamp here: the header's must hold
  void put(uint32_t at, uint32_t byte) { out[at] = (uint8_t)byte; }
  void copy_match(uint32_t at, uint32_t dist, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) out[at + i] = out[at - dist + (dist < len ? i % dist : i)];
  }
  void copy_stored(uint32_t at, uint32_t pos, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) out[at + i] = in[pos + i];
  }
};

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s CORPUS_DIR\n", argv[0]);
    return 2;
  }
  std::vector<std::string> paths;
  for (const auto& e : std::filesystem::directory_iterator(argv[1]))
    if (e.path().extension() == ".bin") paths.push_back(e.path().string());
  std::sort(paths.begin(), paths.end());
  long files = 0, bad = 0, ok0 = 0, compared = 0, pinned_n = 0, by_bit[5] = {0, 0, 0, 0, 0};
  uint64_t worst_iters = 0, worst_bound = 0;
  auto lit = std::make_unique<inf::Huff>(), dst = std::make_unique<inf::Huff>();
  for (const std::string& p : paths) {
    std::ifstream f(p, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (raw.size() < 7) {
      std::fprintf(stderr, "%s: short corpus file\n", p.c_str());
      return 2;
    }
    uint32_t T;
    std::memcpy(&T, raw.data(), 4);
    const int expect = (uint8_t)raw[4], pinned = (uint8_t)raw[5];
    const size_t head = 7 + (raw[6] ? (size_t)T : 0);
    if (raw.size() < head) {
      std::fprintf(stderr, "%s: short corpus file\n", p.c_str());
      return 2;
    }
    const uint8_t* want = raw[6] ? (const uint8_t*)raw.data() + 7 : nullptr;
    const uint32_t size = (uint32_t)(raw.size() - head);
    std::unique_ptr<uint8_t[]> in(new uint8_t[size]), out(new uint8_t[T]), lens(new uint8_t[inf::kLensSize]);
    std::memcpy(in.get(), raw.data() + head, size);
    std::memset(out.get(), 0, T);
    HostEnv env{in.get(), size, out.get(), T};
    uint32_t adler = 0;
    uint64_t iters = 0;
    int st = inf::inflate_stream(env, *lit, *dst, lens.get(), size, T, &adler, &iters);
    if (st == 0) {
      uint64_t s1 = 0, s2 = 0;
      for (uint32_t i = 0; i < T; ++i) {
        s1 += out[i];
        s2 += (uint64_t)(T - i) * out[i];
      }
      if (inf::adler_from_sums((uint32_t)(s1 % 65521), (uint32_t)(s2 % 65521), T) != adler) st |= inf::kStAdler;
    }
    const uint64_t bound = 8ull * size + 1;
    if (iters > worst_iters) worst_iters = iters, worst_bound = bound;
    ++files;
    ok0 += st == 0;
    for (int k = 0; k < 5; ++k) by_bit[k] += (st >> k) & 1;
    if (iters > bound) {
      std::printf("FAIL %s: %llu loop iterations, bound %llu\n", p.c_str(), (unsigned long long)iters, (unsigned long long)bound);
      ++bad;
    }
    if ((st != 0) != (expect != 0)) {
      std::printf("FAIL %s: status %d, zlib %s\n", p.c_str(), st, expect ? "refuses it" : "takes it");
      ++bad;
    }
    if (pinned != 255 && st != pinned) {
      std::printf("FAIL %s: status %d, expected exactly %d\n", p.c_str(), st, pinned);
      ++bad;
    }
    if (want && (st != 0 || std::memcmp(out.get(), want, T) != 0)) {
      std::printf("FAIL %s: the output differs from zlib's bytes\n", p.c_str());
      ++bad;
    }
    compared += want != nullptr;
    pinned_n += pinned != 255;
  }
  std::printf("%ld streams: %ld status 0; bits 1/2/4/8: %ld %ld %ld %ld; most loop iterations %llu (bound %llu); %ld outputs compared with "
              "zlib's bytes; %ld exact statuses; %ld failures\n",
              files, ok0, by_bit[0], by_bit[1], by_bit[2], by_bit[3], (unsigned long long)worst_iters, (unsigned long long)worst_bound,
              compared, pinned_n, bad);
  return bad ? 1 : 0;
}
