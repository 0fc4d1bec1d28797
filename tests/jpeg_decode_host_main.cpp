// The JPEG parser and the entropy decoder of one restart interval (deblurgs_amd/csrc/jpeg_decode_core.h -- the text the
// entropy kernel is compiled from) as a plain host program.  tests/test_jpeg_decode_host.py builds it with
// -fsanitize=address,undefined and runs it over a file of cases it writes:
//
//   u32 n, then per case: u32 kind, u32 file_bytes, u32 n_coef, the file, n_coef int16
//     kind 0   the coefficients must equal the n_coef stored ones
//     kind 1   the parser accepts the file and an interval ends with the status stored in n_coef
//   u32 n_truncate: every truncation length of the first n_truncate cases is parsed and, where accepted, decoded -- as it
//            is (the parser refuses it: no EOI) and with an EOI appended (a scan that stops short: the decoder's business)
//   u32 n_mutate, u32 seed: so many single-byte mutations of every case, from a fixed generator
//
// Every buffer is a heap block of exactly the size the library is told, so a read or write one byte outside is a report.
// A truncated or mutated file may be refused or decoded to anything; it may not make the sanitizers speak.  Exit 0 and a
// line of counts, or 1 and the reason.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../deblurgs_amd/csrc/jpeg_decode_core.h"

namespace {

struct Counts {
  long parsed = 0, unsupported = 0, corrupt = 0, decoded = 0, stopped = 0;
};

// plan + decode of every interval into an exactly-sized buffer; returns the parser's code, the largest status in *status
int run(const uint8_t* bytes, size_t size, std::vector<int16_t>* coef_out, int* status, Counts& n) {
  uint8_t* file = static_cast<uint8_t*>(malloc(size ? size : 1));      // (malloc: aligned for the word loads, exact size)
  memcpy(file, bytes, size);
  JdParse o;
  JdTables t;
  int rc = jd_parse_headers(file, size, o, t);
  void* plan = nullptr;
  if (rc == DGS_OK) {
    const size_t need = jd_plan_bytes(o.n_intervals);
    plan = malloc(need);
    const char* why = "";
    rc = jd_parse(file, size, plan, need, &why);
  }
  if (rc == DGS_E_JPEG_UNSUPPORTED) n.unsupported++;
  else if (rc != DGS_OK) n.corrupt++;
  *status = 0;
  if (rc == DGS_OK) {
    n.parsed++;
    const DgsJpegPlan* p = static_cast<const DgsJpegPlan*>(plan);
    JdGeometry g;
    if (!jd_plan_fits(*p, p->w, p->h, p->channels, g)) {
      fprintf(stderr, "the parser's own plan does not fit\n");
      exit(1);
    }
    int16_t* coef = static_cast<int16_t*>(calloc((size_t)g.total * 64u, sizeof(int16_t)));
    for (int32_t i = 0; i < p->n_intervals; i++) {
      const int s = jd_decode_interval(*p, g, jd_interval_table(p), p->huff, file, (uint32_t)i, coef);
      if (s > *status) *status = s;
    }
    if (*status == 0) n.decoded++;
    else n.stopped++;
    if (coef_out != nullptr) coef_out->assign(coef, coef + (size_t)g.total * 64u);
    free(coef);
  }
  free(plan);
  free(file);
  return rc;
}

uint32_t read_u32(FILE* f) {
  uint32_t v = 0;
  if (fread(&v, 4, 1, f) != 1) {
    fprintf(stderr, "short case file\n");
    exit(1);
  }
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
    return 1;
  }
  FILE* f = fopen(argv[1], "rb");
  if (f == nullptr) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 1;
  }
  const uint32_t n = read_u32(f);
  std::vector<std::vector<uint8_t>> files(n);
  Counts fixtures, truncated, mutated;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t kind = read_u32(f), size = read_u32(f), n_coef = read_u32(f);
    files[i].resize(size);
    std::vector<int16_t> want(kind == 0 ? n_coef : 0);
    if ((size && fread(files[i].data(), 1, size, f) != size) ||
        (!want.empty() && fread(want.data(), 2, want.size(), f) != want.size())) {
      fprintf(stderr, "short case file\n");
      return 1;
    }
    std::vector<int16_t> got;
    int status = 0;
    const int rc = run(files[i].data(), size, &got, &status, fixtures);
    if (rc != DGS_OK) {
      fprintf(stderr, "case %u: the parser refused it (%d)\n", i, rc);
      return 1;
    }
    if (kind == 0 && (status != 0 || got != want)) {
      fprintf(stderr, "case %u: status %d, coefficients %s\n", i, status, got == want ? "equal" : "differ");
      return 1;
    }
    if (kind == 1 && status != (int)n_coef) {
      fprintf(stderr, "case %u: status %d, expected %u\n", i, status, n_coef);
      return 1;
    }
  }
  const uint32_t n_truncate = read_u32(f), n_mutate = read_u32(f);
  uint32_t state = read_u32(f);
  fclose(f);
  for (uint32_t i = 0; i < n_truncate && i < n; i++)
    for (size_t len = 0; len < files[i].size(); len++) {
      int status;
      run(files[i].data(), len, nullptr, &status, truncated);
      std::vector<uint8_t> ended(files[i].begin(), files[i].begin() + len);      // the same with EOI in place: past the parser
      ended.push_back(0xFF);
      ended.push_back(0xD9);
      run(ended.data(), ended.size(), nullptr, &status, truncated);
    }
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t m = 0; m < n_mutate; m++) {
      state ^= state << 13;       // xorshift32
      state ^= state >> 17;
      state ^= state << 5;
      std::vector<uint8_t> copy = files[i];
      copy[state % copy.size()] = (uint8_t)(state >> 24);
      int status;
      run(copy.data(), copy.size(), nullptr, &status, mutated);
    }
  printf("fixtures %ld decoded %ld stopped | truncations %ld parsed %ld corrupt %ld stopped | mutations %ld parsed %ld "
         "unsupported %ld corrupt %ld decoded %ld stopped\n",
         fixtures.decoded, fixtures.stopped, truncated.parsed, truncated.corrupt, truncated.stopped, mutated.parsed,
         mutated.unsupported, mutated.corrupt, mutated.decoded, mutated.stopped);
  return 0;
}
