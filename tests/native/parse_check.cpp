// parse_check.cpp -- every entry of bear_amd/csrc/bear_parse.cpp called from a program of its own, for the host sanitizers
// (`make -C bear_amd/csrc parse-check` builds it three times: address + undefined, thread, address with failing thread creation).
// It writes its inputs into the scratch directory given as its argument, compares what the entries return across thread counts
// and against the naive parser / formatter / encoder below, and exits non-zero on any difference.  Not part of the pytest suite and
// not a GPU program: it is run by hand on a CPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/bear_hip.h"

#ifdef BEAR_PARSE_TEST_THREAD_FAILS_AT
static const int FAILS_AT = BEAR_PARSE_TEST_THREAD_FAILS_AT;   // run_chunks cannot create thread FAILS_AT: more chunks than that fail
#else
static const int FAILS_AT = 0;
#endif
static const bool THREADS_FAIL = FAILS_AT > 0;

static int n_checks = 0, n_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    ++n_checks;                                                             \
    if (!(cond)) {                                                          \
      ++n_failed;                                                           \
      fprintf(stderr, "parse_check.cpp:%d: %s  [%s]\n", __LINE__, #cond, what.c_str()); \
    }                                                                       \
  } while (0)

static std::string dir, what;
static std::string put_file(const char *name, const std::string &text) {
  const std::string path = dir + "/" + name;
  FILE *fh = fopen(path.c_str(), "wb");
  if (!fh || fwrite(text.data(), 1, text.size(), fh) != text.size() || fclose(fh) != 0) {
    fprintf(stderr, "cannot write %s\n", path.c_str());
    exit(2);
  }
  return path;
}
static std::string get_file(const std::string &path) {
  std::string s;
  FILE *fh = fopen(path.c_str(), "rb");
  char buf[65536];
  for (size_t n; fh && (n = fread(buf, 1, sizeof buf, fh)) > 0;) s.append(buf, n);
  if (fh) fclose(fh);
  return s;
}
static void set_threads(int nt) {
  const std::string s = std::to_string(nt);
  setenv("BEAR_PARSE_THREADS", s.c_str(), 1);
  what = s + " threads";
}
static uint64_t rnd_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) {   // xorshift64
  rnd_state ^= rnd_state << 13;
  rnd_state ^= rnd_state >> 7;
  rnd_state ^= rnd_state << 17;
  return (uint32_t)((rnd_state >> 20) % n);
}

// ---------------------------------------------------------------- naive table: generator, formatter, parser
struct table {
  int lag = 0, num_ds = 0, width = 0;
  std::vector<std::string> kmers;
  std::vector<std::vector<uint32_t>> rows;   // [row][ds * width + b]
  size_t n() const { return rows.size(); }
  std::vector<char> planar_kmers() const {
    std::vector<char> k;
    for (const std::string &s : kmers) k.insert(k.end(), s.begin(), s.end());
    return k;
  }
  std::vector<uint32_t> planar_counts() const {
    std::vector<uint32_t> c((size_t)num_ds * n() * width);
    for (size_t r = 0; r < n(); ++r)
      for (int d = 0; d < num_ds; ++d)
        for (int b = 0; b < width; ++b) c[((size_t)d * n() + r) * width + b] = rows[r][d * width + b];
    return c;
  }
};
static table make_table(size_t n, int lag, int num_ds, int width) {
  table t;
  t.lag = lag, t.num_ds = num_ds, t.width = width;
  for (size_t r = 0; r < n; ++r) {
    std::string k;
    for (int i = 0; i < lag; ++i) k += "ACGT["[rnd(5)];
    t.kmers.push_back(k);
    std::vector<uint32_t> row;
    for (int i = 0; i < num_ds * width; ++i) row.push_back(rnd(50) ? rnd(1000) : 4000000000u + rnd(1000));
    t.rows.push_back(row);
  }
  return t;
}
static std::string format_row(const table &t, size_t r) {
  std::string s = t.kmers[r] + "\t[";
  for (int d = 0; d < t.num_ds; ++d) {
    s += d ? ",[" : "[";
    for (int b = 0; b < t.width; ++b) s += (b ? "," : "") + std::to_string(t.rows[r][d * t.width + b]);
    s += "]";
  }
  return s + "]\n";
}
// The text of a table as files in the wild have it: CRLF on some lines, blank lines, no newline behind the last row.
static std::string messy_text(const table &t) {
  std::string s;
  for (size_t r = 0; r < t.n(); ++r) {
    std::string row = format_row(t, r);
    if (r % 7 == 3) row.insert(row.size() - 1, "\r");
    s += row;
    if (r % 1001 == 500) s += r % 2 ? "\n" : " \t\r\n";
  }
  s.pop_back();
  return s;
}
static bool naive_blank(const std::string &l) { return l.find_first_not_of(" \r\t") == std::string::npos; }
static std::vector<std::string> naive_lines(const std::string &text) {
  std::vector<std::string> lines;
  for (size_t p = 0; p < text.size();) {
    size_t nl = text.find('\n', p);
    if (nl == std::string::npos) nl = text.size();
    lines.push_back(text.substr(p, nl - p));
    p = nl + 1;
  }
  return lines;
}
static table naive_parse(const std::string &text, size_t skip, int num_ds, int width) {
  table t;
  t.num_ds = num_ds, t.width = width;
  const std::vector<std::string> lines = naive_lines(text);
  for (size_t i = skip; i < lines.size(); ++i) {
    const std::string &l = lines[i];
    if (naive_blank(l)) continue;
    const size_t tab = l.find('\t');
    t.kmers.push_back(l.substr(0, tab));
    t.lag = (int)tab;
    std::vector<uint32_t> row;
    for (size_t q = tab; q < l.size();) {
      if (l[q] < '0' || l[q] > '9') {
        ++q;
        continue;
      }
      uint64_t v = 0;
      for (; q < l.size() && l[q] >= '0' && l[q] <= '9'; ++q) v = v * 10 + (uint64_t)(l[q] - '0');
      row.push_back((uint32_t)v);
    }
    t.rows.push_back(row);
  }
  return t;
}
static bool naive_member(uint64_t g, uint64_t N, uint64_t B, uint64_t W, uint64_t r) {   // dist.shard_rows per batch
  const uint64_t a = g / B * B, m = N - a < B ? N - a : B, base = m / W, extra = m % W;
  const uint64_t lo = r * base + (r < extra ? r : extra), hi = lo + base + (r < extra ? 1 : 0);
  return g - a >= lo && g - a < hi;
}

// ---------------------------------------------------------------- the table entries
// what every entry that runs nt chunks returns in this build, whatever its input
static int threaded(int nt) { return THREADS_FAIL && nt > FAILS_AT ? BEAR_ERR_NOMEM : BEAR_OK; }

static void check_rows(const table &want, const std::vector<size_t> &idx, size_t max_rows, const char *km, const uint32_t *cn) {
  bool same = true;
  for (size_t o = 0; o < idx.size() && same; ++o) {
    const size_t r = idx[o];
    if (km && memcmp(km + o * want.lag, want.kmers[r].data(), (size_t)want.lag) != 0) same = false;
    for (int d = 0; d < want.num_ds; ++d)
      for (int b = 0; b < want.width; ++b)
        if (cn[((size_t)d * max_rows + o) * want.width + b] != want.rows[r][d * want.width + b]) same = false;
  }
  CHECK(same);
}

static void check_tables(int width, size_t n) {
  const int lag = 7, num_ds = 2;
  const table gen = make_table(n, lag, num_ds, width);
  const std::string body = messy_text(gen), header = "kmer\tcounts\r\n";
  const table want = naive_parse(header + body, 1, num_ds, width);
  what = "width " + std::to_string(width);
  CHECK(body.size() > (1u << 20) && body.size() < (3u << 19));
  CHECK(want.n() == n && want.kmers == gen.kmers && want.rows == gen.rows && want.lag == lag);
  const std::string plain = put_file("plain.tsv", body), headed = put_file("headed.tsv", header + body);
  std::vector<std::string> bad_lines = naive_lines(body);
  size_t mid = bad_lines.size() / 2;
  while (naive_blank(bad_lines[mid])) ++mid;
  bad_lines[mid].replace(lag + 1, 2, "[[x");
  std::string bad_text;
  for (const std::string &l : bad_lines) bad_text += l + "\n";
  const std::string bad = put_file("bad.tsv", bad_text);
  uint64_t newlines = 0;
  for (char c : header + body) newlines += c == '\n';
  std::vector<size_t> all(n);
  for (size_t r = 0; r < n; ++r) all[r] = r;

  for (int nt : {1, 3, 8}) {
    set_threads(nt);
    what += ", width " + std::to_string(width);
    const int thr = threaded(nt);
    uint64_t got = 77, got2 = 77;
    CHECK(bear_count_rows(headed.c_str(), &got) == thr && (thr || got == n + 1));
    CHECK(bear_count_newlines(headed.c_str(), &got) == thr && (thr || got == newlines));
    // the plain reader: whole, without k-mers, clipped, and with a malformed row in the middle
    std::vector<char> km(n * lag, 'x');
    std::vector<uint32_t> cn((size_t)num_ds * n * width, 0xEEEEEEEEu);
    int st = width == 5 ? bear_parse_counts_tsv(plain.c_str(), num_ds, lag, n, km.data(), cn.data(), &got)
                        : bear_parse_counts_tsv_wide(plain.c_str(), num_ds, width, lag, n, km.data(), cn.data(), &got);
    CHECK(st == thr && (thr || got == n));
    if (!thr) check_rows(want, all, n, km.data(), cn.data());
    std::vector<uint32_t> roomy((size_t)num_ds * (n + 5) * width);
    st = bear_parse_counts_tsv_wide(plain.c_str(), num_ds, width, lag, n + 5, nullptr, roomy.data(), &got);
    CHECK(st == thr && (thr || got == n));
    if (!thr) check_rows(want, all, n + 5, nullptr, roomy.data());
    const size_t clip = n * 2 / 3 + 1;
    std::vector<uint32_t> cc((size_t)num_ds * clip * width);   // exactly max_rows rows: a row too many is a heap overflow
    std::vector<char> kc(clip * lag);
    st = bear_parse_counts_tsv_wide(plain.c_str(), num_ds, width, lag, clip, kc.data(), cc.data(), &got);
    CHECK(st == thr && (thr || got == clip));
    if (!thr) check_rows(want, std::vector<size_t>(all.begin(), all.begin() + clip), clip, kc.data(), cc.data());
    st = bear_parse_counts_tsv_wide(bad.c_str(), num_ds, width, lag, n, km.data(), cn.data(), &got);
    CHECK(st == (thr ? thr : BEAR_ERR_PARSE));
    CHECK(bear_parse_counts_tsv_wide(bad.c_str(), num_ds, width, lag, 100, km.data(), cn.data(), &got) == thr && (thr || got == 100));
    // the sharded reader behind the header: every rank's rows, the file's row count, its refusals
    const uint64_t B = 1000, W = 3;
    std::vector<int> seen(n, 0);
    for (uint64_t r = 0; r < W; ++r) {
      std::vector<size_t> idx;
      for (size_t g = 0; g < n; ++g)
        if (naive_member(g, n, B, W, r)) idx.push_back(g), ++seen[g];
      CHECK(bear_shard_rows_count(0, n, n, B, (int)r, (int)W, &got) == BEAR_OK && got == idx.size());
      std::vector<char> ks(idx.size() * lag);
      std::vector<uint32_t> cs((size_t)num_ds * idx.size() * width);
      got = got2 = 77;
      st = width == 5 ? bear_parse_counts_tsv_shard(headed.c_str(), num_ds, lag, 1, 0, n, B, (int)r, (int)W, idx.size(), ks.data(), cs.data(), &got, &got2)
                      : bear_parse_counts_tsv_shard_wide(headed.c_str(), num_ds, width, lag, 1, 0, n, B, (int)r, (int)W, idx.size(), ks.data(),
                                                         cs.data(), &got, &got2);
      CHECK(st == thr && (thr || (got == idx.size() && got2 == n)));
      if (!thr) check_rows(want, idx, idx.size(), ks.data(), cs.data());
      got2 = 77;
      st = bear_parse_counts_tsv_shard_wide(headed.c_str(), num_ds, width, lag, 1, 0, n - 1, B, (int)r, (int)W, idx.size(), ks.data(), cs.data(), &got, &got2);
      CHECK(st == (thr ? thr : BEAR_ERR_INVALID_ARG) && (thr || got2 == n));   // more rows than the caller said: the count is still reported
      st = bear_parse_counts_tsv_shard_wide(headed.c_str(), num_ds, width, lag, 1, 0, n, B, (int)r, (int)W, idx.size() - 1, ks.data(), cs.data(), &got, nullptr);
      CHECK(st == (thr ? thr : BEAR_ERR_INVALID_ARG));
    }
    for (size_t g = 0; g < n; ++g)
      if (seen[g] != 1) seen[0] = -1;
    CHECK(seen[0] == 1);
    st = bear_parse_counts_tsv_shard_wide(bad.c_str(), num_ds, width, lag, 0, 0, n, B, 0, 1, n, km.data(), cn.data(), &got, &got2);
    CHECK(st == (thr ? thr : BEAR_ERR_PARSE));
  }
  what = "table arguments";
  uint64_t got;
  std::vector<uint32_t> cn((size_t)num_ds * n * width);
  CHECK(bear_parse_counts_tsv_wide(plain.c_str(), num_ds, 7, lag, n, nullptr, cn.data(), &got) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_parse_counts_tsv_shard_wide(plain.c_str(), num_ds, 7, lag, 0, 0, n, 10, 0, 1, n, nullptr, cn.data(), &got, nullptr) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_parse_counts_tsv_shard(plain.c_str(), num_ds, lag, 0, 0, n, 10, 2, 2, n, nullptr, cn.data(), &got, nullptr) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_parse_counts_tsv(nullptr, num_ds, lag, n, nullptr, cn.data(), &got) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_parse_counts_tsv((dir + "/absent").c_str(), num_ds, lag, n, nullptr, cn.data(), &got) == BEAR_ERR_IO);
  CHECK(bear_count_rows(nullptr, &got) == BEAR_ERR_INVALID_ARG && bear_count_newlines((dir + "/absent").c_str(), &got) == BEAR_ERR_IO);
}

static void check_empty_file() {
  what = "empty file";
  const std::string path = put_file("empty", "");
  uint64_t a = 7, b = 7;
  uint32_t cn[10];
  char km[4];
  uint8_t text[4];
  CHECK(bear_count_rows(path.c_str(), &a) == BEAR_OK && a == 0);
  a = 7;
  CHECK(bear_count_newlines(path.c_str(), &a) == BEAR_OK && a == 0);
  a = 7;
  CHECK(bear_parse_counts_tsv(path.c_str(), 2, 2, 1, km, cn, &a) == BEAR_OK && a == 0);
  a = 7;
  CHECK(bear_parse_counts_tsv_shard(path.c_str(), 2, 2, 1, 0, 0, 5, 0, 2, 1, km, cn, &a, &b) == BEAR_OK && a == 0 && b == 0);
  a = 7;
  CHECK(bear_parse_sparse_counts(path.c_str(), 2, 5, 2, 1, 1, km, cn, &a) == BEAR_OK && a == 0);
  a = b = 7;
  CHECK(bear_fastx_size(path.c_str(), 0, 1, &a, &b) == BEAR_OK && a == 0 && b == 0);
  a = 7;
  CHECK(bear_fastx_encode(path.c_str(), 1, 1, 0, 4, text, nullptr, &a) == BEAR_OK && a == 0);
}

// ---------------------------------------------------------------- the writer
static void check_writer() {
  const table t = make_table(3 * 65536 + 17, 5, 2, 5), t21 = make_table(300, 3, 1, 21);
  const std::vector<char> km = t.planar_kmers(), km21 = t21.planar_kmers();
  const std::vector<uint32_t> cn = t.planar_counts(), cn21 = t21.planar_counts();
  std::string whole, halves, wide;
  for (size_t r = 0; r < t.n(); ++r) whole += format_row(t, r);
  for (size_t j = 0; j < 2; ++j)
    for (size_t r = j; r < t.n(); r += 2) halves += format_row(t, r);
  for (size_t r = 0; r < t21.n(); ++r) wide += format_row(t21, r);
  const std::string path = dir + "/written.tsv";
  for (int nt : {1, 3, 8}) {
    set_threads(nt);
    const int thr = threaded(nt);   // 3 and 4 writer threads
    CHECK(bear_write_counts_tsv(path.c_str(), km.data(), cn.data(), t.n(), t.lag, t.num_ds, 0, 1, 0) == thr);
    CHECK(thr || get_file(path) == whole);
    CHECK(bear_write_counts_tsv(path.c_str(), km.data(), cn.data(), t.n(), t.lag, t.num_ds, 0, 2, 0) == BEAR_OK);   // 98 313 rows: two ranges
    CHECK(bear_write_counts_tsv(path.c_str(), km.data(), cn.data(), t.n(), t.lag, t.num_ds, 1, 2, 1) == BEAR_OK);
    CHECK(get_file(path) == halves);
    CHECK(bear_write_counts_tsv_wide(path.c_str(), km21.data(), cn21.data(), t21.n(), t21.lag, 1, 21, 0, 1, 0) == BEAR_OK && get_file(path) == wide);
  }
  what = "writer arguments";
  CHECK(bear_write_counts_tsv_wide(path.c_str(), km21.data(), cn21.data(), t21.n(), t21.lag, 1, 7, 0, 1, 0) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_write_counts_tsv(path.c_str(), km.data(), cn.data(), t.n(), t.lag, t.num_ds, 0, 0, 0) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_write_counts_tsv((dir + "/no/such/dir").c_str(), km.data(), cn.data(), 10, t.lag, t.num_ds, 0, 1, 0) == BEAR_ERR_IO);
  CHECK(bear_write_counts_tsv(path.c_str(), km.data(), cn.data(), 10, t.lag, t.num_ds, 20, 1, 0) == BEAR_OK && get_file(path).empty());
}

// ---------------------------------------------------------------- the sparse reader
static void check_sparse() {
  what = "sparse";
  const std::string good =
      "kmer;idx;val\n"
      "ACG; [[0, 0], [1, 4]]; [3, 4000000000]\r\n"
      "\n"
      " [AC ;[[1,2]];[7.0]\n"
      "TTT; []; []";
  const std::string path = put_file("sparse.txt", good);
  char km[9];
  uint32_t cn[2 * 3 * 5];
  uint64_t got = 0;
  CHECK(bear_parse_sparse_counts(path.c_str(), 2, 5, 3, 1, 3, km, cn, &got) == BEAR_OK && got == 3);
  CHECK(memcmp(km, "ACG[ACTTT", 9) == 0);
  uint32_t want[2 * 3 * 5] = {0};
  want[0] = 3, want[(1 * 3 + 0) * 5 + 4] = 4000000000u, want[(1 * 3 + 1) * 5 + 2] = 7;
  CHECK(memcmp(cn, want, sizeof want) == 0);
  CHECK(bear_parse_sparse_counts(path.c_str(), 2, 5, 3, 1, 2, km, cn, &got) == BEAR_OK && got == 2);   // stops at max_rows
  CHECK(bear_parse_sparse_counts(path.c_str(), 2, 5, 3, 1, 3, nullptr, cn, &got) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_parse_sparse_counts(path.c_str(), 2, 5, 3, 0, 3, km, cn, &got) == BEAR_ERR_PARSE);         // the header is no row
  const char *refused[] = {"ACG; [[0, 0]]",            "ACGT; [[0, 0]]; [1]",   "ACG; [[0, 0], [1]]; [1]", "ACG; [[0, -]]; [1]",
                           "ACG; [[2, 0]]; [1]",       "ACG; [[0, 5]]; [1]",    "ACG; [[0, 0]]; [-1]",     "ACG; [[0, 0]]; [1.5]",
                           "ACG; [[0, 0]]; [1, 2]",    "ACG; [[0, 0], [1, 1]]; [1]", "ACG; [[0, 0]]; [4294967296]", "ACG; [[0, 0]]; [.]"};
  for (const char *row : refused) {
    what = std::string("sparse refusal: ") + row;
    const std::string p = put_file("sparse_bad.txt", std::string("TTT; [[0, 1]]; [2]\n") + row);
    CHECK(bear_parse_sparse_counts(p.c_str(), 2, 5, 3, 0, 3, km, cn, &got) == BEAR_ERR_PARSE);
  }
}

// ---------------------------------------------------------------- the binary cache
static void check_cache() {
  what = "cache";
  const table t = make_table(1000, 6, 3, 5);
  const std::vector<char> km = t.planar_kmers();
  const std::vector<uint32_t> cn = t.planar_counts();
  const std::string path = dir + "/table.cache", src = put_file("cache_src", "abc");
  uint64_t size = 0, n = 0, ssize = 0;
  int64_t mtime = 0, smtime = 0;
  int lag = 0, num_ds = 0;
  CHECK(bear_stat_source(src.c_str(), &size, &mtime) == BEAR_OK && size == 3 && mtime > 0);
  CHECK(bear_stat_source((dir + "/absent").c_str(), &size, &mtime) == BEAR_ERR_IO);
  CHECK(bear_cache_write(path.c_str(), km.data(), cn.data(), t.n(), t.lag, t.num_ds, size, mtime) == BEAR_OK);
  CHECK(bear_cache_info(path.c_str(), &n, &lag, &num_ds, &ssize, &smtime) == BEAR_OK);
  CHECK(n == t.n() && lag == t.lag && num_ds == t.num_ds && ssize == size && smtime == mtime);
  std::vector<char> k2(100 * 6);
  std::vector<uint32_t> c2(3 * 100 * 5);
  CHECK(bear_cache_read(path.c_str(), 900, 100, k2.data(), c2.data()) == BEAR_OK);
  std::vector<size_t> idx;
  for (size_t r = 900; r < 1000; ++r) idx.push_back(r);
  check_rows(t, idx, 100, k2.data(), c2.data());
  CHECK(bear_cache_read(path.c_str(), 901, 100, k2.data(), c2.data()) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_cache_read((dir + "/absent").c_str(), 0, 1, k2.data(), c2.data()) == BEAR_ERR_IO);
  std::string raw = get_file(path);
  put_file("table.cache", "XXXX" + raw.substr(4));
  CHECK(bear_cache_info(path.c_str(), &n, nullptr, nullptr, nullptr, nullptr) == BEAR_ERR_PARSE);
  put_file("table.cache", raw.substr(0, raw.size() - 1));   // truncated
  CHECK(bear_cache_read(path.c_str(), 0, 1, k2.data(), c2.data()) == BEAR_ERR_PARSE);
}

// ---------------------------------------------------------------- FASTA / FASTQ
struct record_text {   // the naive encoder: one record's characters, already joined and trimmed
  std::vector<uint8_t> text;
  uint64_t seqs = 0;
  void add(std::string s, int width, bool reverse) {
    const std::string letters = width == 5 ? "ACGT" : "ARNDCEQGHILKMFPSTWYV";
    if (width == 21 && !s.empty() && s.back() == '*') s.pop_back();
    std::vector<uint8_t> codes;
    for (char c : s) {
      const size_t i = letters.find((char)(c >= 'a' && c <= 'z' ? c - 32 : c));
      codes.push_back(i == std::string::npos ? (uint8_t)(width + 1) : (uint8_t)i);
    }
    text.push_back((uint8_t)width);
    text.insert(text.end(), codes.begin(), codes.end());
    text.push_back((uint8_t)(width - 1));
    ++seqs;
    if (!reverse) return;
    text.push_back(5);
    for (size_t i = codes.size(); i-- > 0;) text.push_back(codes[i] < 4 ? (uint8_t)(3 - codes[i]) : codes[i]);
    text.push_back(4);
    ++seqs;
  }
};
static void check_fastx_file(const std::string &file_text, int fastq, int width, int reverse, const std::vector<std::string> &records) {
  record_text want;
  for (const std::string &r : records) want.add(r, width, reverse != 0);
  const std::string path = put_file("seqs", file_text);
  uint64_t n_pos = 0, n_seqs = 0, n_enc = 0;
  CHECK(bear_fastx_size_wide(path.c_str(), fastq, reverse, width, &n_pos, &n_seqs) == BEAR_OK);
  CHECK(n_pos == want.text.size() && n_seqs == want.seqs);
  std::vector<uint8_t> text(want.text.size()), group(want.text.size());   // exactly the capacity: one code too many is a heap overflow
  CHECK(bear_fastx_encode_wide(path.c_str(), fastq, reverse, width, 3, text.size(), text.data(), group.data(), &n_enc) == BEAR_OK);
  CHECK(n_enc == want.text.size() && text == want.text && group == std::vector<uint8_t>(group.size(), 3));
  if (width == 5) {
    std::vector<uint8_t> t5(text.size());
    n_pos = n_enc = 0;
    CHECK(bear_fastx_size(path.c_str(), fastq, reverse, &n_pos, nullptr) == BEAR_OK && n_pos == want.text.size());
    CHECK(bear_fastx_encode(path.c_str(), fastq, reverse, 0, t5.size(), t5.data(), nullptr, &n_enc) == BEAR_OK && t5 == want.text);
  }
  for (size_t cap : {text.size() - 1, text.size() / 2, (size_t)0}) {   // a capacity that is too small: refused, nothing written beyond it
    std::vector<uint8_t> small(cap + 1);
    CHECK(bear_fastx_encode_wide(path.c_str(), fastq, reverse, width, 3, cap, small.data(), nullptr, &n_enc) == BEAR_ERR_INVALID_ARG);
  }
}
static void check_fastx() {
  what = "FASTA dna";
  const std::string fasta = "; a comment in front of the first record\n>r1 first\nACGTN\r\n  acgt \n\n>r2 empty\n>r3\nGATTACA\n>r4\nT";
  const std::vector<std::string> dna = {"ACGTNacgt", "", "GATTACA", "T"};
  check_fastx_file(fasta, 0, 5, 0, dna);
  check_fastx_file(fasta, 0, 5, 1, dna);
  what = "FASTQ dna";
  const std::string fastq = "@q1\nACGTN\n+\nIIIII\n\n@q2\r\nGGC*A\r\n+q2\r\nIIIII\r\n@q3\n\n+\n\n@q4\nTTA\n+\nII";
  const std::vector<std::string> reads = {"ACGTN", "GGC*A", "", "TTA"};
  check_fastx_file(fastq, 1, 5, 0, reads);
  check_fastx_file(fastq, 1, 5, 1, reads);
  what = "FASTA protein";
  const std::string prot = ">p1 stop at the end\nMKV*\n>p2 stop in the middle\nMK*VL\n>p3 stop at the end of a line\nMKV*\nLLX\n>p4 two stops\nAR**\n>p5 only a stop\n*\n>p6\nwy*\r\n";
  const std::vector<std::string> prots = {"MKV*", "MK*VL", "MKV*LLX", "AR**", "*", "wy*"};
  check_fastx_file(prot, 0, 21, 0, prots);
  what = "FASTQ protein";
  check_fastx_file("@a\nMKV*\n+\nIIII\n@b\nM*K\n+\nIII\n", 1, 21, 0, {"MKV*", "M*K"});
  what = "fastx refusals";
  const std::string path = put_file("seqs", fasta), broken = put_file("broken.fq", "@q1\nACGT\nIIII\n"), cut = put_file("cut.fq", "@q1\nACGT\n+\n");
  uint64_t a = 0, b = 0;
  uint8_t text[64];
  CHECK(bear_fastx_size_wide(path.c_str(), 0, 1, 21, &a, &b) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_fastx_size_wide(path.c_str(), 0, 0, 7, &a, &b) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_fastx_encode_wide(path.c_str(), 0, 1, 21, 0, 64, text, nullptr, &a) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_fastx_encode_wide(path.c_str(), 0, 0, 5, 255, 64, text, nullptr, &a) == BEAR_ERR_INVALID_ARG);
  CHECK(bear_fastx_size(broken.c_str(), 1, 0, &a, &b) == BEAR_ERR_PARSE && bear_fastx_encode(broken.c_str(), 1, 0, 0, 64, text, nullptr, &a) == BEAR_ERR_PARSE);
  CHECK(bear_fastx_size(cut.c_str(), 1, 0, &a, &b) == BEAR_ERR_PARSE && bear_fastx_size(path.c_str(), 1, 0, &a, &b) == BEAR_ERR_PARSE);
  CHECK(bear_fastx_size((dir + "/absent").c_str(), 0, 0, &a, &b) == BEAR_ERR_IO && bear_fastx_size(nullptr, 0, 0, &a, &b) == BEAR_ERR_INVALID_ARG);
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]);
    return 2;
  }
  dir = argv[1];
  check_tables(5, 22000);
  check_tables(21, 6500);
  check_writer();
  unsetenv("BEAR_PARSE_THREADS");
  check_empty_file();
  check_sparse();
  check_cache();
  check_fastx();
  printf("parse_check%s: %d checks, %d failed\n", THREADS_FAIL ? " (thread creation fails)" : "", n_checks, n_failed);
  return n_failed ? 1 : 0;
}
