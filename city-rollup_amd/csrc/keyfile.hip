// libcityprover_hip.so, fourth translation unit: Groth16 keys as files.
// A key is saved once, after the setup, and loaded without the trapdoor: cp_groth16_key_save_file, cp_groth16_key_load_file,
// cp_groth16_key_file_info. The file is little-endian u64 words; word i counts from the start of the file:
//   0          magic: the bytes "CPG16KEY"
//   1          version (1)
//   2          checksum
//   3          flags (bit 0: raw points; every other bit 0)
//   4, 5, 6    log_domain, n_wires, n_public
//   7          0
//   8 .. 115   alpha_g1[12], beta_g1[12], delta_g1[12], beta_g2[24], delta_g2[24], gamma_g2[24]: affine canonical
//   next       IC: n_public x 12 words (affine canonical), then n_public flag bytes zero-padded to a whole word
//   then       a_g1 (n_wires points), b_g1 (n_wires), b_g2 (n_wires), k_g1 (n_wires - n_public), z_g1 (2^log_domain - 1)
// A point of the five sets is a compressed element - 48 bytes (G1) or 96 (G2: a0, then a1 with the flags on a1), the encoding
// bls_sqrt.h decodes for stored proofs: x little-endian, 0x80 on the last byte where y is the larger root, 0x40 alone for
// infinity - or, in a raw file, 96 / 192 bytes of affine canonical coordinates with all-zero coordinates for infinity.
// Infinity is allowed in a_g1, b_g1 and b_g2 (their flag arrays are rebuilt from it; b_g1[i] and b_g2[i] must agree) and
// refused in k_g1 and z_g1, for which cp_groth16_pk has no flags. The header determines the length exactly.
// checksum = sum mod 2^64 over every word i != 2 of mix(w_i ^ i * 0x9E3779B97F4A7C15), mix the splitmix64 finaliser: free of
// order, so every chunk is summed on its own. It is summed on the host: the bytes pass through host memory on their way to
// or from the file, and it is verified before any point is looked at.
//
// The points are packed and unpacked on the device, one lane per point, in passes of chunk_points through one staging buffer on
// the device and two page-locked ones on the host: the host reads (or writes) one pass while the device works on its neighbour.
#include "core.h"
#include "groth16_keyfile.h"
#include "groth16_key.h"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <unistd.h>

namespace keyfile {

constexpr unsigned LANES = 64;  // one wave per workgroup, as the unpack kernels of pairing.hip
// what a set does with the point at infinity
enum { INF_REFUSED = 0, INF_WRITES_FLAG = 1, INF_MATCHES_FLAG = 2 };

// Internal form plus flag -> the file's form (pack_point). Point i of this pass is pts[i] / inf[i] and goes to out + i * point words.
template <class F>
__global__ __launch_bounds__(LANES) void k_pack(const AffineT<F> *__restrict__ pts, const uint8_t *__restrict__ inf, size_t n, int raw,
                                                uint32_t *__restrict__ out) {
  constexpr int W = Field<F>::WORDS;
  const size_t i = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (i >= n) return;
  pack_point<F>(pts[i], inf && inf[i], raw != 0, out + i * (raw ? 2 * W : W));
}

// The file's form -> internal form plus flag, straight into the key's arrays. Point i of this pass is point base + i of its set:
// unpack_point of src + i * point words -> out[i], inf[i] (out and inf already point at entry `base`). A refused point puts
// (base + i) * 8 + class into *first_bad through a minimum: the lowest refused index of the pass, and why. An entry that is
// infinity, or refused, holds `gen`, as the setup leaves the generator under a flag.
template <class F>
__global__ __launch_bounds__(LANES) void k_unpack(const uint32_t *__restrict__ src, size_t n, size_t base, int raw, int inf_mode, AffineT<F> gen,
                                                  AffineT<F> *__restrict__ out, uint8_t *__restrict__ inf, unsigned long long *__restrict__ first_bad) {
  constexpr int W = Field<F>::WORDS;
  const size_t i = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (i >= n) return;
  const uint32_t *s = src + i * (raw ? 2 * W : W);
  AffineT<F> a = gen;
  bool is_inf = false;
  int st = unpack_point<F>(s, raw != 0, a, is_inf);
  if (st == ST_OK && is_inf && inf_mode == INF_REFUSED) st = ST_INFINITY;
  if (st == ST_OK && inf_mode == INF_MATCHES_FLAG && (inf[i] != 0) != is_inf) st = ST_DISAGREE;
  if (st != ST_OK) atomicMin(first_bad, (unsigned long long)(base + i) * 8 + (unsigned)st);
  if (inf_mode == INF_WRITES_FLAG) inf[i] = is_inf ? 1 : 0;
  out[i] = (st != ST_OK || is_inf) ? gen : a;
}

// CP_GROTH16_KEY_LOAD_CHECK_TORSION, behind k_unpack on the stream and in a launch of its own (the 255 doublings want twice the
// registers of a root): [r] pts[i] = infinity for the entries of the pass as they now stand in the key's array. The generator
// under a flag, or in place of a refused point, passes.
template <class F>
__global__ __launch_bounds__(LANES) void k_torsion(const AffineT<F> *__restrict__ pts, size_t n, size_t base, unsigned long long *__restrict__ first_bad) {
  const size_t i = (size_t)blockIdx.x * LANES + threadIdx.x;
  if (i >= n) return;
  if (!pairing::in_r_torsion(pts[i])) atomicMin(first_bad, (unsigned long long)(base + i) * 8 + (unsigned)ST_TORSION);
}

// ---- the file on the host ----
constexpr uint64_t MAGIC = 0x59454B3631475043ull;  // "CPG16KEY"
constexpr size_t FIXED_WORDS = 116;                // the header and the six single points
constexpr size_t DEFAULT_CHUNK = (size_t)1 << 16;  // points per pass: 12 MiB of staging at the widest point

inline uint64_t mix(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// the checksum's sum over n words that start at word `first` of the file (word 2, the checksum itself, does not count)
uint64_t checksum_words(const uint64_t *w, size_t n, uint64_t first) {
  uint64_t s = 0;
  for (size_t k = 0; k < n; k++)
    if (first + k != 2) s += mix(w[k] ^ ((first + k) * 0x9E3779B97F4A7C15ull));
  return s;
}

// the same over a large span: pieces of 2^16 words on a few short-lived threads (the sum is free of order)
uint64_t checksum_span(const uint64_t *w, size_t n, uint64_t first) {
  constexpr size_t PIECE = (size_t)1 << 16;
  const size_t pieces = (n + PIECE - 1) / PIECE;
  if (pieces < 4) return checksum_words(w, n, first);
  std::vector<uint64_t> part(pieces, 0);
  unsigned hw = std::thread::hardware_concurrency();
  hostu::parallel_for(pieces, std::min<size_t>(8, hw ? hw : 1), [&](size_t p) {
    part[p] = checksum_words(w + p * PIECE, std::min(PIECE, n - p * PIECE), first + p * PIECE);
  });
  uint64_t s = 0;
  for (uint64_t v : part) s += v;
  return s;
}

enum { SET_A = 0, SET_B1, SET_B2, SET_K, SET_Z, N_SETS };
const char *const SET_NAMES[N_SETS] = {"a_g1", "b_g1", "b_g2", "k_g1", "z_g1"};

// where everything is, from the four numbers of the header (all in u64 words)
struct Layout {
  bool raw = false;
  int log_domain = 0;
  size_t n_wires = 0, n_public = 0;
  size_t ic_off = FIXED_WORDS, ic_flag_off = 0;
  size_t set_off[N_SETS] = {}, set_n[N_SETS] = {}, set_point_words[N_SETS] = {};
  size_t total_words = 0;
  void fill() {
    ic_flag_off = ic_off + 12 * n_public;
    size_t off = ic_flag_off + (n_public + 7) / 8;
    const size_t counts[N_SETS] = {n_wires, n_wires, n_wires, n_wires - n_public, ((size_t)1 << log_domain) - 1};
    for (int s = 0; s < N_SETS; s++) {
      set_off[s] = off;
      set_n[s] = counts[s];
      set_point_words[s] = (s == SET_B2 ? 12 : 6) * (raw ? 2 : 1);
      off += counts[s] * set_point_words[s];
    }
    total_words = off;
  }
};

// the ranges every reader and the writer hold a header to; nullptr = fine
const char *layout_problem(uint64_t flags, uint64_t log_domain, uint64_t n_wires, uint64_t n_public) {
  if (flags & ~(uint64_t)CP_GROTH16_KEY_FILE_RAW) return "a reserved flag bit is set";
  if (log_domain == 0 || log_domain > 28) return "log_domain out of range (1 .. 28)";
  if (n_wires == 0 || n_wires > ((uint64_t)1 << 28)) return "n_wires out of range (1 .. 2^28)";
  if (n_public == 0 || n_public > n_wires) return "n_public out of range (1 .. n_wires)";
  return nullptr;
}

struct File {
  FILE *f = nullptr;
  ~File() { if (f) fclose(f); }
};

struct Parsed {
  Layout lay;
  uint64_t checksum = 0;
  size_t file_bytes = 0;
  cp_groth16_vk vk{};
  uint64_t beta_g1[12], delta_g1[12];
  std::vector<uint64_t> ic_xy;
  std::vector<uint8_t> ic_inf;
};

int io_error(cp_ctx *ctx, int code, const char *what, const char *path) {
  const int e = errno;
  return set_error(ctx, code, "%s %s: %s", what, path, e ? strerror(e) : "unexpected end of file");
}

// Opens the file and checks everything that needs no square root: structure, version, sizes, the exact length, the header's
// points being canonical, and - asked for - the checksum over the whole file. The file stays open in `file`.
int parse(cp_ctx *ctx, const char *path, bool verify_checksum, Parsed *out, File *file) {
  hostu::alloc_checkpoint();
  errno = 0;
  file->f = fopen(path, "rb");
  if (!file->f) return io_error(ctx, CP_ERR_INVALID_ARG, "cannot open key file", path);
  FILE *f = file->f;
  if (fseek(f, 0, SEEK_END) != 0) return io_error(ctx, CP_ERR_INVALID_ARG, "cannot seek in", path);
  const long end = ftell(f);
  if (end < 0) return io_error(ctx, CP_ERR_INVALID_ARG, "cannot seek in", path);
  rewind(f);
  const size_t bytes = (size_t)end;
  uint64_t head[FIXED_WORDS];
  if (bytes < sizeof head) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: truncated header (%zu bytes)", path, bytes);
  if (fread(head, 8, FIXED_WORDS, f) != FIXED_WORDS) return io_error(ctx, CP_ERR_INTERNAL, "cannot read", path);
  if (head[0] != MAGIC) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: not a Groth16 key file (bad magic)", path);
  if (head[1] != CP_GROTH16_KEY_FILE_VERSION)
    return set_error(ctx, CP_ERR_UNSUPPORTED, "%s: key file version %llu (this library reads version %d)", path, (unsigned long long)head[1], CP_GROTH16_KEY_FILE_VERSION);
  if (const char *why = layout_problem(head[3], head[4], head[5], head[6])) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: %s", path, why);
  if (head[7] != 0) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: word 7 of the header is not zero", path);
  Parsed &P = *out;
  Layout &L = P.lay;
  L.raw = (head[3] & CP_GROTH16_KEY_FILE_RAW) != 0;
  L.log_domain = (int)head[4];
  L.n_wires = (size_t)head[5];
  L.n_public = (size_t)head[6];
  L.fill();
  if (bytes != L.total_words * 8)
    return set_error(ctx, CP_ERR_INVALID_ARG, "%s: the file has %zu bytes, its header needs %zu", path, bytes, L.total_words * 8);
  P.checksum = head[2];
  P.file_bytes = bytes;
  const size_t ic_words = L.set_off[0] - FIXED_WORDS;  // points and flag words
  std::vector<uint64_t> ic(ic_words);
  if (fread(ic.data(), 8, ic_words, f) != ic_words) return io_error(ctx, CP_ERR_INTERNAL, "cannot read", path);
  if (verify_checksum) {
    uint64_t sum = checksum_words(head, FIXED_WORDS, 0) + checksum_words(ic.data(), ic_words, FIXED_WORDS);
    std::vector<uint64_t> block(std::min(L.total_words - L.set_off[0] + 1, (size_t)1 << 22));  // at most 32 MiB at a time
    size_t at = L.set_off[0];
    while (at < L.total_words) {
      const size_t n = std::min(block.size(), L.total_words - at);
      if (fread(block.data(), 8, n, f) != n) return io_error(ctx, CP_ERR_INTERNAL, "cannot read", path);
      sum += checksum_span(block.data(), n, at);
      at += n;
    }
    if (sum != P.checksum) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: checksum mismatch (corrupt file)", path);
  }
  // the header's points: canonical here, the curve and the subgroup where a verifier is made of them
  const struct { const char *name; size_t off, coords; } fixed[] = {{"alpha_g1", 8, 2},  {"beta_g1", 20, 2},  {"delta_g1", 32, 2},
                                                                   {"beta_g2", 44, 4},  {"delta_g2", 68, 4}, {"gamma_g2", 92, 4}};
  for (const auto &p : fixed)
    for (size_t c = 0; c < p.coords; c++)
      if (!pairing::words_below_p((const uint32_t *)(head + p.off + 6 * c)))
        return set_error(ctx, CP_ERR_INVALID_ARG, "%s: %s has a coordinate that is not canonical (>= p)", path, p.name);
  for (size_t i = 0; i < 2 * L.n_public; i++)
    if (!pairing::words_below_p((const uint32_t *)(ic.data() + 6 * i)))
      return set_error(ctx, CP_ERR_INVALID_ARG, "%s: ic[%zu] has a coordinate that is not canonical (>= p)", path, i / 2);
  const uint8_t *icf = (const uint8_t *)(ic.data() + 12 * L.n_public);
  for (size_t i = 0; i < 8 * ((L.n_public + 7) / 8); i++)
    if (icf[i] > (i < L.n_public ? 1 : 0)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: the IC flag bytes hold something other than 0 / 1 and zero padding", path);
  memcpy(P.vk.alpha_g1, head + 8, 96);
  memcpy(P.beta_g1, head + 20, 96);
  memcpy(P.delta_g1, head + 32, 96);
  memcpy(P.vk.beta_g2, head + 44, 192);
  memcpy(P.vk.delta_g2, head + 68, 192);
  memcpy(P.vk.gamma_g2, head + 92, 192);
  P.vk.n_public = L.n_public;
  P.ic_xy.assign(ic.begin(), ic.begin() + 12 * L.n_public);
  P.ic_inf.assign(icf, icf + L.n_public);
  return CP_OK;
}

// one device pass: `count` points of set `set` from point `base` on
struct Pass { int set; size_t base, count; };
std::vector<Pass> passes_of(const Layout &L, size_t chunk) {
  std::vector<Pass> v;
  for (int s = 0; s < N_SETS; s++)
    for (size_t b = 0; b < L.set_n[s]; b += chunk) v.push_back({s, b, std::min(chunk, L.set_n[s] - b)});
  return v;
}
// the staging of a call: one device buffer and two page-locked ones of chunk points at the widest form, and the chunk itself
struct Staging {
  size_t chunk = 0;
  uint64_t *dev = nullptr;
  PinBuf pin[2];
  uint64_t *host(size_t k) const { return pin[k & 1].get<uint64_t>(); }
};
int staging_alloc(cp_ctx *ctx, const Layout &L, size_t chunk_points, DevBag &tmp, Staging &st) {
  size_t most = 1;
  for (int s = 0; s < N_SETS; s++) most = std::max(most, L.set_n[s]);
  st.chunk = std::min(chunk_points ? chunk_points : DEFAULT_CHUNK, most);
  const size_t bytes = st.chunk * L.set_point_words[SET_B2] * 8;
  CP_TRY(alloc_status(ctx, tmp.alloc(&st.dev, bytes), bytes));
  for (PinBuf &p : st.pin) {
    p = PinBuf(pin_pool(), ctx->device);
    CP_TRY(alloc_status(ctx, p.alloc(bytes), bytes));
  }
  return CP_OK;
}

// the generators in the internal form: what an entry under an infinity flag holds
template <class F> AffineT<F> generator();
template <> AffineT<Fp> generator<Fp>() { return bls::affine_from_canonical<Fp>((const uint32_t *)BLS_G1_GEN); }
template <> AffineT<Fp2> generator<Fp2>() { return bls::affine_from_canonical<Fp2>((const uint32_t *)BLS_G2_GEN); }

const char *class_text(int st) {
  switch (st) {
    case ST_FLAG: return "has a flag bit set that may not be set";
    case ST_RANGE: return "has a coordinate that is not canonical (>= p)";
    case ST_NO_POINT: return "is no point of the curve";
    case ST_INFINITY: return "is the point at infinity, which this set cannot hold";
    case ST_DISAGREE: return "and b_g1 of the same wire disagree about the point at infinity";
    default: return "is outside the r-torsion subgroup";
  }
}

int load_run(cp_ctx *ctx, const char *path, unsigned flags, size_t chunk_points, cp_groth16_key *key) {
  Parsed P;
  File file;
  CP_TRY(parse(ctx, path, true, &P, &file));
  const Layout &L = P.lay;
  const size_t m = L.n_wires, n_private = m - L.n_public, flag_bytes = (m + 7) & ~(size_t)7;
  // the arrays of the key, sized as the setup sizes them
  void *sets[N_SETS];
  uint8_t *a_inf = nullptr, *b_inf = nullptr;
  const size_t set_bytes[N_SETS] = {m * CP_G1_AFFINE_BYTES, m * CP_G1_AFFINE_BYTES, m * CP_G2_AFFINE_BYTES, (n_private ? n_private : 1) * CP_G1_AFFINE_BYTES,
                                    L.set_n[SET_Z] * CP_G1_AFFINE_BYTES};
  for (int s = 0; s < N_SETS; s++) CP_TRY(alloc_status(ctx, key->mem.alloc(&sets[s], set_bytes[s]), set_bytes[s]));
  CP_TRY(alloc_status(ctx, key->mem.alloc(&a_inf, flag_bytes), flag_bytes));
  CP_TRY(alloc_status(ctx, key->mem.alloc(&b_inf, flag_bytes), flag_bytes));
  unsigned long long bad = 0;  // declared in this order: the bag waits for the stream when it dies, before the page-locked
  Staging st;                  // buffers and the word that queued copies may still write
  DevBag tmp = ctx->bag();
  unsigned long long *first_bad = nullptr;
  CP_TRY(staging_alloc(ctx, L, chunk_points, tmp, st));
  CP_TRY(alloc_status(ctx, tmp.alloc(&first_bad, 8), 8));
  HIP_TRY(ctx, hipMemsetAsync(a_inf, 0, flag_bytes, ctx->stream));  // the padding of the last word
  HIP_TRY(ctx, hipMemsetAsync(b_inf, 0, flag_bytes, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(first_bad, 0xff, 8, ctx->stream));
  const AffineT<Fp> g1 = generator<Fp>();
  const AffineT<Fp2> g2 = generator<Fp2>();
  const int torsion = (flags & CP_GROTH16_KEY_LOAD_CHECK_TORSION) ? 1 : 0, raw = L.raw ? 1 : 0;
  const std::vector<Pass> passes = passes_of(L, st.chunk);
  FILE *f = file.f;
  auto read_pass = [&](size_t k) -> int {  // the file's bytes of pass k into its page-locked buffer
    const Pass &p = passes[k];
    const size_t pw = L.set_point_words[p.set];
    if (fseek(f, (long)((L.set_off[p.set] + p.base * pw) * 8), SEEK_SET) != 0 || fread(st.host(k), 8, p.count * pw, f) != p.count * pw)
      return io_error(ctx, CP_ERR_INTERNAL, "cannot read", path);
    return CP_OK;
  };
  errno = 0;
  if (!passes.empty()) CP_TRY(read_pass(0));
  for (size_t k = 0; k < passes.size(); k++) {
    const Pass &p = passes[k];
    const size_t pw = L.set_point_words[p.set];
    HIP_TRY(ctx, hipMemcpyAsync(st.dev, st.host(k), p.count * pw * 8, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid(blocks_for(p.count, LANES)), block(LANES);
    if (p.set == SET_B2) {
      AffineT<Fp2> *out = (AffineT<Fp2> *)sets[p.set] + p.base;
      LAUNCH(ctx, "keyfile_unpack_g2", k_unpack<Fp2>, grid, block, (const uint32_t *)st.dev, p.count, p.base, raw, (int)INF_MATCHES_FLAG, g2, out, b_inf + p.base,
             first_bad);
      if (torsion) LAUNCH(ctx, "keyfile_torsion_g2", k_torsion<Fp2>, grid, block, (const AffineT<Fp2> *)out, p.count, p.base, first_bad);
    } else {
      AffineT<Fp> *out = (AffineT<Fp> *)sets[p.set] + p.base;
      uint8_t *inf = p.set == SET_A ? a_inf + p.base : p.set == SET_B1 ? b_inf + p.base : nullptr;
      LAUNCH(ctx, "keyfile_unpack_g1", k_unpack<Fp>, grid, block, (const uint32_t *)st.dev, p.count, p.base, raw, (int)(inf ? INF_WRITES_FLAG : INF_REFUSED), g1, out, inf,
             first_bad);
      if (torsion) LAUNCH(ctx, "keyfile_torsion_g1", k_torsion<Fp>, grid, block, (const AffineT<Fp> *)out, p.count, p.base, first_bad);
    }
    HIP_TRY(ctx, hipMemcpyAsync(&bad, first_bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    const int next = k + 1 < passes.size() ? read_pass(k + 1) : CP_OK;  // under the kernel
    HIP_TRY(ctx, sync_stream(ctx));
    CP_TRY(next);
    if (bad != ~0ull)
      return set_error(ctx, CP_ERR_INVALID_ARG, "%s: %s[%llu] %s", path, SET_NAMES[p.set], bad >> 3, class_text((int)(bad & 7)));
  }
  cp_groth16_pk &pk = key->pk;
  pk.n_wires = m;
  pk.n_private = n_private;
  pk.log_domain = L.log_domain;
  pk.a_g1 = sets[SET_A]; pk.b_g1 = sets[SET_B1]; pk.b_g2 = sets[SET_B2]; pk.k_g1 = sets[SET_K]; pk.z_g1 = sets[SET_Z];
  pk.a_inf = a_inf; pk.b_inf = b_inf;
  memcpy(pk.alpha_g1, P.vk.alpha_g1, 96);
  memcpy(pk.beta_g1, P.beta_g1, 96);
  memcpy(pk.delta_g1, P.delta_g1, 96);
  memcpy(pk.beta_g2, P.vk.beta_g2, 192);
  memcpy(pk.delta_g2, P.vk.delta_g2, 192);
  key->vk = P.vk;
  key->ic_xy = std::move(P.ic_xy);
  key->ic_inf = std::move(P.ic_inf);
  return CP_OK;
}

// the temporary file of a save: gone again unless the save got as far as the rename
struct TempFile {
  std::string name;
  FILE *f = nullptr;
  ~TempFile() {
    if (f) fclose(f);
    if (!name.empty()) (void)unlink(name.c_str());
  }
};

int save_run(cp_ctx *ctx, const cp_groth16_key *key, const char *path, unsigned flags, size_t chunk_points) {
  hostu::alloc_checkpoint();
  const cp_groth16_pk &pk = key->pk;
  Layout L;
  L.raw = (flags & CP_GROTH16_KEY_FILE_RAW) != 0;
  L.log_domain = pk.log_domain;
  L.n_wires = pk.n_wires;
  L.n_public = key->vk.n_public;
  if (const char *why = layout_problem(flags & CP_GROTH16_KEY_FILE_RAW, (uint64_t)pk.log_domain, pk.n_wires, L.n_public)) return set_error(ctx, CP_ERR_INVALID_ARG, "save: the key's %s", why);
  L.fill();
  static std::atomic<unsigned> serial{0};
  TempFile out;
  out.name = std::string(path) + ".tmp." + std::to_string((long)getpid()) + "." + std::to_string(serial.fetch_add(1));
  errno = 0;
  out.f = fopen(out.name.c_str(), "wb");
  if (!out.f) {
    const int rc = io_error(ctx, CP_ERR_INVALID_ARG, "cannot create", out.name.c_str());
    out.name.clear();  // nothing was created
    return rc;
  }
  // the header, the six single points and the IC, with the checksum word still zero
  std::vector<uint64_t> head(L.set_off[0], 0);
  head[0] = MAGIC;
  head[1] = CP_GROTH16_KEY_FILE_VERSION;
  head[3] = L.raw ? CP_GROTH16_KEY_FILE_RAW : 0;
  head[4] = (uint64_t)L.log_domain;
  head[5] = L.n_wires;
  head[6] = L.n_public;
  memcpy(&head[8], pk.alpha_g1, 96);
  memcpy(&head[20], pk.beta_g1, 96);
  memcpy(&head[32], pk.delta_g1, 96);
  memcpy(&head[44], pk.beta_g2, 192);
  memcpy(&head[68], pk.delta_g2, 192);
  memcpy(&head[92], key->vk.gamma_g2, 192);
  memcpy(&head[L.ic_off], key->ic_xy.data(), 96 * L.n_public);
  for (size_t i = 0; i < L.n_public; i++) ((uint8_t *)&head[L.ic_flag_off])[i] = key->ic_inf[i] ? 1 : 0;
  uint64_t sum = checksum_words(head.data(), head.size(), 0);
  if (fwrite(head.data(), 8, head.size(), out.f) != head.size()) return io_error(ctx, CP_ERR_INTERNAL, "cannot write", out.name.c_str());
  Staging st;  // before the bag, which waits for the stream when it dies: no copy is still writing a page-locked buffer that is freed
  DevBag tmp = ctx->bag();
  CP_TRY(staging_alloc(ctx, L, chunk_points, tmp, st));
  const void *sets[N_SETS] = {pk.a_g1, pk.b_g1, pk.b_g2, pk.k_g1, pk.z_g1};
  const std::vector<Pass> passes = passes_of(L, st.chunk);
  const int raw = L.raw ? 1 : 0;
  auto write_pass = [&](size_t k) -> int {  // pass k from its page-locked buffer to the file; the sets follow each other in pass order
    const Pass &p = passes[k];
    const size_t pw = L.set_point_words[p.set], n = p.count * pw;
    sum += checksum_span(st.host(k), n, L.set_off[p.set] + p.base * pw);
    if (fwrite(st.host(k), 8, n, out.f) != n) return io_error(ctx, CP_ERR_INTERNAL, "cannot write", out.name.c_str());
    return CP_OK;
  };
  for (size_t k = 0; k < passes.size(); k++) {
    const Pass &p = passes[k];
    const size_t pw = L.set_point_words[p.set];
    const dim3 grid(blocks_for(p.count, LANES)), block(LANES);
    if (p.set == SET_B2) {
      LAUNCH(ctx, "keyfile_pack_g2", k_pack<Fp2>, grid, block, (const AffineT<Fp2> *)sets[p.set] + p.base, pk.b_inf + p.base, p.count, raw, (uint32_t *)st.dev);
    } else {
      const uint8_t *inf = p.set == SET_A ? pk.a_inf + p.base : p.set == SET_B1 ? pk.b_inf + p.base : nullptr;
      LAUNCH(ctx, "keyfile_pack_g1", k_pack<Fp>, grid, block, (const AffineT<Fp> *)sets[p.set] + p.base, inf, p.count, raw, (uint32_t *)st.dev);
    }
    HIP_TRY(ctx, hipMemcpyAsync(st.host(k), st.dev, p.count * pw * 8, hipMemcpyDeviceToHost, ctx->stream));
    const int prev = k > 0 ? write_pass(k - 1) : CP_OK;  // under the kernel
    HIP_TRY(ctx, sync_stream(ctx));
    CP_TRY(prev);
  }
  if (!passes.empty()) CP_TRY(write_pass(passes.size() - 1));
  if (fseek(out.f, 16, SEEK_SET) != 0 || fwrite(&sum, 8, 1, out.f) != 1 || fflush(out.f) != 0) return io_error(ctx, CP_ERR_INTERNAL, "cannot write", out.name.c_str());
  FILE *f = out.f;
  out.f = nullptr;
  if (fclose(f) != 0) return io_error(ctx, CP_ERR_INTERNAL, "cannot write", out.name.c_str());
  if (rename(out.name.c_str(), path) != 0) return io_error(ctx, CP_ERR_INTERNAL, "cannot rename the temporary file to", path);
  out.name.clear();
  return CP_OK;
}

}  // namespace keyfile

extern "C" {

int cp_groth16_key_save_file(cp_ctx *ctx, const cp_groth16_key *key, const char *path, unsigned flags, size_t chunk_points) try {
  CHECK_CTX(ctx);
  if (!key || !path) return set_error(ctx, CP_ERR_INVALID_ARG, "save: NULL argument");
  if (flags & ~CP_GROTH16_KEY_FILE_RAW) return set_error(ctx, CP_ERR_INVALID_ARG, "save: unknown flag bits 0x%x", flags);
  if (key->device != ctx->device) return set_error(ctx, CP_ERR_INVALID_ARG, "save: the key lives on device %d, the context on device %d", key->device, ctx->device);
  return keyfile::save_run(ctx, key, path, flags, chunk_points);
} CP_CATCH(ctx)

cp_groth16_key *cp_groth16_key_load_file(cp_ctx *ctx, const char *path, unsigned flags, size_t chunk_points) try {
  if (!ctx) { set_error(nullptr, CP_ERR_INVALID_ARG, "ctx is NULL"); return nullptr; }
  if (!path) { set_error(ctx, CP_ERR_INVALID_ARG, "load: path is NULL"); return nullptr; }
  if (flags & ~CP_GROTH16_KEY_LOAD_CHECK_TORSION) { set_error(ctx, CP_ERR_INVALID_ARG, "load: unknown flag bits 0x%x", flags); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  cp_groth16_key *key = new cp_groth16_key(ctx->device);
  struct Guard { cp_groth16_key *k; ~Guard() { groth16_key_free(k); } } guard{key};
  if (keyfile::load_run(ctx, path, flags, chunk_points, key) != CP_OK) return nullptr;
  guard.k = nullptr;
  return key;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

int cp_groth16_key_file_info(const char *path, int verify_checksum, struct cp_groth16_key_file_info *info_out, cp_groth16_vk *vk_out, uint64_t *ic_xy_out,
                             uint8_t *ic_inf_out) try {
  if (!path) return set_error(nullptr, CP_ERR_INVALID_ARG, "path is NULL");
  keyfile::Parsed P;
  keyfile::File file;
  CP_TRY(keyfile::parse(nullptr, path, verify_checksum != 0, &P, &file));
  if (info_out) {
    info_out->version = CP_GROTH16_KEY_FILE_VERSION;
    info_out->flags = P.lay.raw ? CP_GROTH16_KEY_FILE_RAW : 0;
    info_out->log_domain = P.lay.log_domain;
    info_out->n_wires = P.lay.n_wires;
    info_out->n_public = P.lay.n_public;
    info_out->n_private = P.lay.n_wires - P.lay.n_public;
    info_out->file_bytes = P.file_bytes;
    info_out->checksum = P.checksum;
  }
  if (vk_out) *vk_out = P.vk;
  if (ic_xy_out) memcpy(ic_xy_out, P.ic_xy.data(), P.ic_xy.size() * 8);
  if (ic_inf_out) memcpy(ic_inf_out, P.ic_inf.data(), P.ic_inf.size());
  return CP_OK;
} CP_CATCH(nullptr)

}  // extern "C"
