// Circuit files (".cpcirc"): one built circuit as flat data — what the Rust side of the bridge (SURVEY.md §8(f) N1) dumps
// from plonky2's `CommonCircuitData` / `ProverOnlyCircuitData` after `CircuitBuilder::build`
// (reference build sites: city_common_circuit/src/proof_minifier/pm_core.rs:96-105,
// city_rollup_circuit/src/worker/toolbox/root.rs:75-139; the fields are the ones the reference itself serialises at
// city_common_circuit/src/verify_template/ser_data.rs:55-123) and what cp_circuit_load_file turns into a resident circuit.
// Layout, little-endian, every section 8-byte aligned (INTEGRATION.md §4 has the same table and the Rust writer):
//   0    char  magic[8] = "CPCIRCv1"
//   8    u32   version = 1
//   12   u32   flags        bit 0: the polynomials are COEFFICIENTS (PolynomialBatch::polynomials), else values over <omega_n>
//                           bit 1: k_is present          bit 2: public-input targets present
//   16   u64   total_bytes  (the whole file, checksum included)
//   24   i32   shape[24]    cp_shape in declaration order: degree_bits, num_constants, num_routed_wires, num_wires,
//                           num_challenges, num_partial_products, quotient_degree_factor, rate_bits, cap_height, pow_bits,
//                           num_query_rounds, n_arity, arity_bits[8], zero_knowledge, num_public_inputs, 0, 0
//   120  u64   circuit_digest[4]
//   152  u32   num_selectors, u32 n_gates
//   160  i32   gates[n_gates][7]   cp_gate: type, selector_index, group_start, group_end, param, param2, param3
//        (+4 bytes of zero padding when n_gates is odd)
//        u64   k_is[num_routed_wires]                      (flag bit 1)
//        u32   public_input_targets[num_public_inputs][2]  (flag bit 2: row, wire of public input j in the wire matrix)
//        u64   polynomials[num_constants + num_routed_wires][n]   constants (selectors first) then sigmas
//   end  u64   FNV-1a 64 of every preceding byte
// Included by cityprover.hip after quotient.inc and prover_tail.inc.

namespace cfile {

constexpr uint32_t FLAG_COEFFS = 1, FLAG_K_IS = 2, FLAG_PI_TARGETS = 4;
constexpr size_t HEADER = 160;

inline uint64_t fnv1a(const uint8_t *p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
  for (size_t i = 0; i < n; i++) {
    h ^= p[i];
    h *= 0x100000001b3ull;
  }
  return h;
}

struct Parsed {
  cp_shape sh;
  uint64_t digest[4];
  uint32_t flags = 0;
  int num_selectors = 0;
  std::vector<cp_gate> gates;
  std::vector<uint64_t> k_is;
  std::vector<uint32_t> pi_targets;  // [num_public_inputs][2]
  size_t polys_offset = 0, n_polys = 0, n = 0;
};

void shape_to_i32(const cp_shape &sh, int32_t v[24]) {
  const int32_t f[24] = {sh.degree_bits, sh.num_constants, sh.num_routed_wires, sh.num_wires, sh.num_challenges, sh.num_partial_products,
                         sh.quotient_degree_factor, sh.rate_bits, sh.cap_height, sh.pow_bits, sh.num_query_rounds, sh.n_arity,
                         sh.arity_bits[0], sh.arity_bits[1], sh.arity_bits[2], sh.arity_bits[3], sh.arity_bits[4], sh.arity_bits[5],
                         sh.arity_bits[6], sh.arity_bits[7], sh.zero_knowledge, sh.num_public_inputs, 0, 0};
  memcpy(v, f, sizeof f);
}
void shape_from_i32(const int32_t v[24], cp_shape *sh) {
  memset(sh, 0, sizeof *sh);
  sh->degree_bits = v[0]; sh->num_constants = v[1]; sh->num_routed_wires = v[2]; sh->num_wires = v[3]; sh->num_challenges = v[4];
  sh->num_partial_products = v[5]; sh->quotient_degree_factor = v[6]; sh->rate_bits = v[7]; sh->cap_height = v[8]; sh->pow_bits = v[9];
  sh->num_query_rounds = v[10]; sh->n_arity = v[11];
  for (int i = 0; i < 8; i++) sh->arity_bits[i] = v[12 + i];
  sh->zero_knowledge = v[20]; sh->num_public_inputs = v[21];
}

// Reads and checks everything but the polynomial values (structure, sizes, checksum over the whole file).
// `keep`: when non-null, receives the whole file (the loader then uploads the polynomials from it).
int parse(cp_ctx *ctx, const char *path, Parsed *out, std::vector<uint8_t> *keep) {
  if (!path) return set_error(ctx, CP_ERR_INVALID_ARG, "path is NULL");
  FILE *f = fopen(path, "rb");
  if (!f) return set_error(ctx, CP_ERR_INVALID_ARG, "cannot open circuit file %s", path);
  struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
  uint8_t head[HEADER];
  if (fread(head, 1, HEADER, f) != HEADER) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: truncated header", path);
  if (memcmp(head, "CPCIRCv1", 8) != 0) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: not a circuit file (bad magic)", path);
  uint32_t version, flags;
  uint64_t total;
  memcpy(&version, head + 8, 4);
  memcpy(&flags, head + 12, 4);
  memcpy(&total, head + 16, 8);
  if (version != 1) return set_error(ctx, CP_ERR_UNSUPPORTED, "%s: circuit file version %u (this library reads version 1)", path, version);
  if (flags & ~(FLAG_COEFFS | FLAG_K_IS | FLAG_PI_TARGETS)) return set_error(ctx, CP_ERR_UNSUPPORTED, "%s: unknown flags 0x%x", path, flags);
  int32_t shv[24];
  memcpy(shv, head + 24, sizeof shv);
  Parsed &P = *out;
  shape_from_i32(shv, &P.sh);
  memcpy(P.digest, head + 120, 32);
  uint32_t nsel, ngates;
  memcpy(&nsel, head + 152, 4);
  memcpy(&ngates, head + 156, 4);
  const cp_shape &sh = P.sh;
  if (shv[22] != 0 || shv[23] != 0) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: shape out of range", path);
  if (const char *why = shape_problem(sh)) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: %s", path, why);
  if (sh.degree_bits > 26) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: shape out of range", path);
  if (ngates > quot::MAX_GATES || nsel > (uint32_t)sh.num_constants) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: bad gate / selector count", path);
  P.flags = flags;
  P.num_selectors = (int)nsel;
  P.n = (size_t)1 << sh.degree_bits;
  P.n_polys = (size_t)sh.num_constants + sh.num_routed_wires;
  size_t off = HEADER + (size_t)ngates * 28;
  off = (off + 7) & ~(size_t)7;
  const size_t k_off = off;
  if (flags & FLAG_K_IS) off += (size_t)sh.num_routed_wires * 8;
  const size_t t_off = off;
  if (flags & FLAG_PI_TARGETS) off += (size_t)sh.num_public_inputs * 8;
  P.polys_offset = off;
  const size_t want_total = off + P.n_polys * P.n * 8 + 8;
  if (total != want_total) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: header says %llu bytes, the shape needs %zu", path, (unsigned long long)total, want_total);
  if (fseek(f, 0, SEEK_END) != 0 || (uint64_t)ftell(f) != total) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: file size differs from the header's total", path);
  rewind(f);
  hostu::alloc_checkpoint();
  std::vector<uint8_t> local;
  std::vector<uint8_t> &buf = keep ? *keep : local;
  buf.resize(total);
  if (fread(buf.data(), 1, total, f) != total) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: short read", path);
  uint64_t sum;
  memcpy(&sum, buf.data() + total - 8, 8);
  if (fnv1a(buf.data(), total - 8) != sum) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: checksum mismatch (corrupt file)", path);
  P.gates.resize(ngates);
  for (uint32_t g = 0; g < ngates; g++) {
    int32_t v[7];
    memcpy(v, buf.data() + HEADER + (size_t)g * 28, 28);
    P.gates[g] = cp_gate{v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
  }
  if (flags & FLAG_K_IS) {
    P.k_is.resize(sh.num_routed_wires);
    memcpy(P.k_is.data(), buf.data() + k_off, P.k_is.size() * 8);
  }
  if (flags & FLAG_PI_TARGETS) {
    P.pi_targets.resize((size_t)2 * sh.num_public_inputs);
    memcpy(P.pi_targets.data(), buf.data() + t_off, P.pi_targets.size() * 4);
    for (int j = 0; j < sh.num_public_inputs; j++)
      if (P.pi_targets[2 * j] >= P.n || P.pi_targets[2 * j + 1] >= (uint32_t)sh.num_wires)
        return set_error(ctx, CP_ERR_INVALID_ARG, "%s: public-input target %d is outside the wire matrix", path, j);
  }
  const uint64_t *polys = (const uint64_t *)(buf.data() + P.polys_offset);
  for (size_t i = 0; i < P.n_polys * P.n; i++) {
    uint64_t v;
    memcpy(&v, polys + i, 8);
    if (v >= gl::P) return set_error(ctx, CP_ERR_INVALID_ARG, "%s: polynomial element %zu is not canonical", path, i);
  }
  return CP_OK;
}

}  // namespace cfile

extern "C" {

int cp_circuit_file_info(const char *path, cp_shape *shape_out, uint64_t digest_out[4], size_t *n_gates_out, int *num_selectors_out,
                         unsigned *flags_out) try {
  cfile::Parsed P;
  CP_TRY(cfile::parse(nullptr, path, &P, nullptr));
  if (shape_out) *shape_out = P.sh;
  if (digest_out) memcpy(digest_out, P.digest, 32);
  if (n_gates_out) *n_gates_out = P.gates.size();
  if (num_selectors_out) *num_selectors_out = P.num_selectors;
  if (flags_out) *flags_out = P.flags;
  return CP_OK;
} CP_CATCH(nullptr)

cp_circuit *cp_circuit_load_file(cp_ctx *ctx, const char *path) try {
  if (!ctx) { set_error(nullptr, CP_ERR_INVALID_ARG, "ctx is NULL"); return nullptr; }
  cfile::Parsed P;
  std::vector<uint8_t> buf;
  if (cfile::parse(ctx, path, &P, &buf) != CP_OK) return nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, CP_ERR_HIP, "hipSetDevice failed"); return nullptr; }
  const uint64_t *polys = (const uint64_t *)(buf.data() + P.polys_offset);
  std::vector<uint64_t> values;
  if (P.flags & cfile::FLAG_COEFFS) {  // coefficient form: one forward NTT per polynomial gives the values the loader wants
    values.resize(P.n_polys * P.n);
    DevBuf tmp = ctx->buf();
    if (alloc_status(ctx, tmp.alloc(values.size() * 8), values.size() * 8) != CP_OK) return nullptr;
    uint64_t *d = tmp.get<uint64_t>();
    if (cp_h2d(ctx, d, polys, values.size() * 8) != CP_OK || cp_ntt_dev(ctx, d, P.sh.degree_bits, P.n_polys, P.n, 0, 0) != CP_OK ||
        cp_d2h(ctx, values.data(), d, values.size() * 8) != CP_OK)
      return nullptr;
    polys = values.data();
  }
  cp_circuit *c = cp_circuit_load(ctx, &P.sh, P.digest, polys, (P.flags & cfile::FLAG_K_IS) ? P.k_is.data() : nullptr);
  if (!c) return nullptr;
  if (cp_circuit_set_gates(c, P.gates.data(), P.gates.size(), P.num_selectors) != CP_OK) {
    cp_circuit_destroy(c);
    return nullptr;
  }
  c->pi_targets = P.pi_targets;
  return c;
} catch (...) {
  exception_status(ctx);
  return nullptr;
}

int cp_circuit_save_file(cp_circuit *c, const char *path) try {
  if (!c || !path) return set_error(c ? c->ctx : nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  cp_ctx *ctx = c->ctx;
  CHECK_CTX(ctx);
  if (!c->has_gates) return set_error(ctx, CP_ERR_INVALID_ARG, "circuit has no gate set (cp_circuit_set_gates)");
  const cp_shape &sh = c->sh;
  const size_t n = (size_t)1 << sh.degree_bits, n_polys = (size_t)sh.num_constants + sh.num_routed_wires;
  const bool targets = !c->pi_targets.empty();
  size_t off = cfile::HEADER + c->gates.size() * 28;
  off = (off + 7) & ~(size_t)7;
  const size_t k_off = off;
  off += (size_t)sh.num_routed_wires * 8;
  const size_t t_off = off;
  if (targets) off += (size_t)sh.num_public_inputs * 8;
  const size_t total = off + n_polys * n * 8 + 8;
  hostu::alloc_checkpoint();
  std::vector<uint8_t> buf(total, 0);
  memcpy(buf.data(), "CPCIRCv1", 8);
  const uint32_t version = 1, flags = cfile::FLAG_K_IS | (targets ? cfile::FLAG_PI_TARGETS : 0);
  const uint64_t total64 = total;
  memcpy(buf.data() + 8, &version, 4);
  memcpy(buf.data() + 12, &flags, 4);
  memcpy(buf.data() + 16, &total64, 8);
  int32_t shv[24];
  cfile::shape_to_i32(sh, shv);
  memcpy(buf.data() + 24, shv, sizeof shv);
  memcpy(buf.data() + 120, c->digest, 32);
  const uint32_t nsel = (uint32_t)c->num_selectors, ngates = (uint32_t)c->gates.size();
  memcpy(buf.data() + 152, &nsel, 4);
  memcpy(buf.data() + 156, &ngates, 4);
  for (uint32_t g = 0; g < ngates; g++) {
    const quot::Gate &q = c->gates[g];
    const int32_t v[7] = {q.type, q.selector_index, q.group_start, q.group_end, q.param, q.param2, q.param3};
    memcpy(buf.data() + cfile::HEADER + (size_t)g * 28, v, 28);
  }
  if (sh.num_routed_wires) CP_TRY(cp_d2h(ctx, buf.data() + k_off, c->k_is, (size_t)sh.num_routed_wires * 8));
  if (targets) memcpy(buf.data() + t_off, c->pi_targets.data(), c->pi_targets.size() * 4);
  CP_TRY(cp_d2h(ctx, buf.data() + off, c->cs_values, n_polys * n * 8));
  const uint64_t sum = cfile::fnv1a(buf.data(), total - 8);
  memcpy(buf.data() + total - 8, &sum, 8);
  FILE *f = fopen(path, "wb");
  if (!f) return set_error(ctx, CP_ERR_INVALID_ARG, "cannot create %s", path);
  const bool ok = fwrite(buf.data(), 1, total, f) == total;
  if (fclose(f) != 0 || !ok) return set_error(ctx, CP_ERR_INTERNAL, "short write to %s", path);
  return CP_OK;
} CP_CATCH(c ? c->ctx : nullptr)

int cp_circuit_set_public_input_targets(cp_circuit *c, const uint32_t *row_wire_pairs, size_t n_targets) try {
  if (!c) return set_error(nullptr, CP_ERR_INVALID_ARG, "circuit is NULL");
  cp_ctx *ctx = c->ctx;
  if (n_targets != (size_t)c->sh.num_public_inputs) return set_error(ctx, CP_ERR_INVALID_ARG, "%zu targets given, the circuit has %d public inputs", n_targets, c->sh.num_public_inputs);
  if (n_targets && !row_wire_pairs) return set_error(ctx, CP_ERR_INVALID_ARG, "targets are NULL");
  for (size_t j = 0; j < n_targets; j++)
    if (row_wire_pairs[2 * j] >= ((uint32_t)1 << c->sh.degree_bits) || row_wire_pairs[2 * j + 1] >= (uint32_t)c->sh.num_wires)
      return set_error(ctx, CP_ERR_INVALID_ARG, "public-input target %zu is outside the wire matrix", j);
  c->pi_targets.assign(row_wire_pairs, row_wire_pairs + 2 * n_targets);
  return CP_OK;
} CP_CATCH(c ? c->ctx : nullptr)

int cp_circuit_public_inputs_from_wires(cp_circuit *c, const uint64_t *wires_values_host, uint64_t *public_inputs_out) try {
  if (!c) return set_error(nullptr, CP_ERR_INVALID_ARG, "circuit is NULL");
  cp_ctx *ctx = c->ctx;
  if (c->sh.num_public_inputs == 0) return CP_OK;
  if (!wires_values_host || !public_inputs_out) return set_error(ctx, CP_ERR_INVALID_ARG, "NULL argument");
  if (c->pi_targets.empty()) return set_error(ctx, CP_ERR_INVALID_ARG, "the circuit carries no public-input targets");
  const size_t n = (size_t)1 << c->sh.degree_bits;
  for (int j = 0; j < c->sh.num_public_inputs; j++)
    public_inputs_out[j] = wires_values_host[(size_t)c->pi_targets[2 * j + 1] * n + c->pi_targets[2 * j]];
  return CP_OK;
} CP_CATCH(c ? c->ctx : nullptr)

int cp_circuit_shape(cp_circuit *c, cp_shape *shape_out, uint64_t digest_out[4]) try {
  if (!c || !shape_out) return set_error(c ? c->ctx : nullptr, CP_ERR_INVALID_ARG, "NULL argument");
  *shape_out = c->sh;
  if (digest_out) memcpy(digest_out, c->digest, 32);
  return CP_OK;
} CP_CATCH(c ? c->ctx : nullptr)

}  // extern "C"
