// Stand-alone AddressSanitizer / UBSan run of the decimal token parser (csrc/parse32.h through
// rpt_decimal_parse_host, csrc/parse32.cpp -- the code the PLY row kernels run per token): the
// edge tokens of the domain, digit strings of every length 0..40 with the point at every place,
// seeded random tokens over the parser's alphabet and beyond it, each token also alone at the very
// end of an exactly sized heap block so that a byte read past it is seen.  Checks: status, ok is
// 0 or 1, an in-domain token reads as float(strtod(token)) and its verdict matches a restatement
// of the domain rules.
//
//   make -C tools/asan parse32
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rpt.h"

static uint64_t next_u64(uint64_t* s) {  // splitmix64
  uint64_t z = (*s += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// the domain, restated on strings: [+-]? digits[.digits*] | .digits ; <= 19 digits without the
// leading zeros, integer <= 2^53, <= 22 digits behind the point
static bool in_domain(const std::string& t) {
  size_t i = 0;
  if (i < t.size() && (t[i] == '+' || t[i] == '-')) ++i;
  std::string digits;
  int points = 0, frac = 0;
  for (; i < t.size(); ++i) {
    if (t[i] == '.') {
      if (++points > 1) return false;
    } else if (t[i] >= '0' && t[i] <= '9') {
      digits.push_back(t[i]);
      frac += points;
    } else {
      return false;
    }
  }
  if (digits.empty() || frac > 22) return false;
  const size_t nz = digits.find_first_not_of('0');
  if (nz == std::string::npos) return true;
  digits = digits.substr(nz);
  if (digits.size() > 19) return false;
  return std::strtoull(digits.c_str(), nullptr, 10) <= (1ull << 53);
}

int main() {
  std::vector<std::string> toks = {
      "0", "-0.000000", "0.000000", "007", ".5", "5.", "+1.5", "-.25", "255", "9007199254740992",
      "9007199254740993", "5.73106837272644", "1234567890123456789", "18446744073709551621",
      "12345678901234567890", "1e5", "1E-3", "nan", "inf", "-inf", "1_0", "1..2", "--1", "+", ".",
      "", "-", "+.", "\xef\xbc\x91", "1 ", " 1", "0.0000000000000000000001",
      "0.00000000000000000000001", "9007199254.740992", "9007199254.740993"};
  toks.push_back(std::string("1\0", 2));
  uint64_t seed = 2053;
  // every length 0..40, the point at every place (and absent), digits seeded
  for (int len = 0; len <= 40; ++len) {
    for (int pt = -1; pt < len; ++pt) {
      for (int lead = 0; lead < 2; ++lead) {
        std::string t;
        for (int k = 0; k < len; ++k) {
          const char digit = lead && k < len / 2 ? '0' : (char)('0' + next_u64(&seed) % 10);
          t.push_back(k == pt ? '.' : digit);
        }
        toks.push_back(t);
        toks.push_back("-" + t);
      }
    }
  }
  const char alphabet[] = "0123456789.+-e_ \t\r\n\x0c\xc3";
  for (int k = 0; k < 20000; ++k) {
    const int len = (int)(next_u64(&seed) % 12);
    std::string t;
    for (int j = 0; j < len; ++j) {
      const uint64_t r = next_u64(&seed);
      const char other = alphabet[(r >> 8) % (sizeof(alphabet) - 1)];
      t.push_back(r % 8 ? (char)('0' + (r >> 8) % 10) : other);
    }
    toks.push_back(t);
  }

  const int64_t n = (int64_t)toks.size();
  size_t total = 0;
  for (const std::string& t : toks) total += t.size();
  // exactly sized heap blocks: the redzone sits right behind the last token's last byte
  char* text = static_cast<char*>(std::malloc(total ? total : 1));
  int64_t* off = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * n));
  int32_t* len = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * n));
  float* out = static_cast<float*>(std::malloc(sizeof(float) * n));
  uint8_t* ok = static_cast<uint8_t*>(std::malloc(n));
  if (!text || !off || !len || !out || !ok) return 2;
  size_t pos = 0;
  for (int64_t i = 0; i < n; ++i) {
    off[i] = (int64_t)pos;
    len[i] = (int32_t)toks[i].size();
    std::memcpy(text + pos, toks[i].data(), toks[i].size());
    pos += toks[i].size();
  }
  std::memset(ok, 7, n);
  if (rpt_decimal_parse_host(text, off, len, n, out, ok) != RPT_OK) {
    std::fprintf(stderr, "parse32_main: rpt_decimal_parse_host failed\n");
    return 1;
  }
  int64_t bad = 0, inside = 0;
  for (int64_t i = 0; i < n; ++i) {
    const std::string& t = toks[i];
    const bool want = in_domain(t);
    bool good = ok[i] == (want ? 1 : 0);
    if (good && want) {
      ++inside;
      const float ref = (float)std::strtod(t.c_str(), nullptr);  // two roundings, as the reference
      good = std::memcmp(&ref, &out[i], sizeof(float)) == 0;
    } else if (good) {
      good = out[i] == 0.0f;
    }
    // the token alone, ending where its heap block ends
    char* own = static_cast<char*>(std::malloc(t.size() ? t.size() : 1));
    if (!own) return 2;
    std::memcpy(own, t.data(), t.size());
    const int64_t zero = 0;
    const int32_t l = (int32_t)t.size();
    float v = -1.0f;
    uint8_t k = 7;
    if (rpt_decimal_parse_host(own, &zero, &l, 1, &v, &k) != RPT_OK || k != ok[i] ||
        std::memcmp(&v, &out[i], sizeof(float)) != 0)
      good = false;
    std::free(own);
    if (!good && bad++ < 10)
      std::fprintf(stderr, "parse32_main: token \"%s\" -> ok %d value %.9g (in domain: %d)\n",
                   t.c_str(), (int)ok[i], (double)out[i], (int)want);
  }
  std::free(text);
  std::free(off);
  std::free(len);
  std::free(out);
  std::free(ok);
  const int32_t neg = -3;
  const int64_t zero = 0;
  float v = 1.0f;
  uint8_t k = 7;
  if (rpt_decimal_parse_host(nullptr, nullptr, nullptr, 0, nullptr, nullptr) != RPT_OK ||
      rpt_decimal_parse_host(nullptr, nullptr, nullptr, 1, nullptr, nullptr) != RPT_EINVAL ||
      rpt_decimal_parse_host("1", &zero, &neg, 1, &v, &k) != RPT_OK || k != 0)
    ++bad;
  std::printf("parse32_main: %lld tokens (%lld inside the domain), %lld bad\n", (long long)n,
              (long long)inside, (long long)bad);
  return bad == 0 && inside > 1000 ? 0 : 1;
}
