/* datetime_ops.h -- per-row logic of the timestamp conversions to and from string columns (reference members
 * NVStrings::timestamp2long / long2timestamp, cpp/src/strings/datetime.cu), restated over a row's bytes.
 *
 * Everything a row needs is `__host__ __device__` (plain inline for a host compiler) so that the kernels of
 * cs_datetime.hip and the CPU harness of tests/test_datetime_cpu.py compile the same text.  The units are a template
 * parameter: every divisor (86400, 86400000, ...) is a compile-time constant, so no 64-bit division is left to a
 * runtime call on the device.
 *
 * The format is compiled once per call on the host (compile_ts_format) into a TsProgram: every specifier sits at a fixed
 * byte offset of the input row (parse) and of the output row (format), so the per-row code walks a short list of
 * specifiers and runs of literal bytes, and every formatted row has the same width W.  The reference's quirks are kept:
 *  - parse: literals are skipped unchecked; a specifier fails the row when 0 <= remaining < width; digits are read up to
 *    the field width, stopping at the first non-digit; %p adds 12 to an hour <= 12 on "PM" (any case); %z is added to the
 *    result; %Z must be "UTC" (any case); a A w b B U W fail the row.  A failed, null or empty row gives 0.
 *  - format: int2str prints the low `width` digits, a value <= 0 as zeros; %I is hour % 12; %p is "AM" when hour <= 12;
 *    %z and a A w b B U W write nothing (W counts only what is written).
 *
 * Two documented deviations:
 *  1. a byte past the end of a row reads as NUL (the reference reads the next object's bytes once a literal has stepped
 *     past the end and its unsigned remaining count has wrapped);
 *  2. signed overflow is 64-bit (int fields: 32-bit) two's-complement wrap, where the reference's behaviour is undefined.
 */
#ifndef CS_DATETIME_OPS_H
#define CS_DATETIME_OPS_H
#include <stdint.h>
#include <string.h>

#include <type_traits>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CSDT_HD __host__ __device__ __forceinline__
#else
#define CSDT_HD static inline
#endif

namespace csdt {

// NVStrings::timestamp_units (NVStrings.h:1128), same values
enum TsUnits { TS_YEARS = 0, TS_MONTHS, TS_DAYS, TS_HOURS, TS_MINUTES, TS_SECONDS, TS_MS, TS_US, TS_NS };

enum TsCompile { TS_OK = 0, TS_ERR_UNFINISHED, TS_ERR_SPECIFIER, TS_ERR_TOO_LONG, TS_ERR_UNITS };

// the program travels in the kernel arguments: bounded
constexpr int kTsMaxItems = 64;   // specifiers and runs of literal bytes
constexpr int kTsMaxLit = 256;    // literal bytes in all
constexpr const char* kTsDefaultFormat = "%Y-%m-%dT%H:%M:%SZ";

struct TsItem {
  char spec;       // the specifier; 0 = a run of literal bytes
  uint8_t width;   // bytes read (parse); for a literal run the run's length
  uint8_t out_w;   // bytes written (format)
  uint8_t pad;
  uint16_t lit;    // literal run: its first byte in TsProgram::lit
  uint16_t pad2;
  int32_t in_off;  // where the item starts in an input row
  int32_t out_off; // ... and in an output row
};
struct TsProgram {
  int32_t count;   // items
  int32_t width;   // W: bytes of every formatted row
  int32_t in_len;  // bytes the format spans in an input row (the reference's template length)
  int32_t units;
  TsItem items[kTsMaxItems];
  char lit[kTsMaxLit];
};

// datetime.cu:78-85 (%f: 3 for ms, 9 for ns); -1 = not a specifier
CSDT_HD int ts_spec_width(char c, int units) {
  switch (c) {
    case 'a': case 'A': case 'b': case 'B': return 0;
    case 'w': return 1;
    case 'Y': return 4;
    case 'y': case 'm': case 'd': case 'H': case 'I': case 'M': case 'S': case 'p': case 'U': case 'W': return 2;
    case 'j': case 'Z': return 3;
    case 'z': return 5;
    case 'f': return units == TS_MS ? 3 : units == TS_NS ? 9 : 6;
    default: return -1;
  }
}
// bytes the specifier writes (datetime_formatter::format_from_parts): z, a A w b B U W write nothing
CSDT_HD int ts_spec_out_width(char c, int width) {
  switch (c) {
    case 'z': case 'a': case 'A': case 'w': case 'b': case 'B': case 'U': case 'W': return 0;
    default: return width;
  }
}

// Compiles `fmt` (nullptr: the default) for `units` (DTFormatCompiler::compile_to_device, datetime.cu:100-143).
inline int compile_ts_format(const char* fmt, int units, TsProgram* prog) {
  if (units < TS_YEARS || units > TS_NS) return TS_ERR_UNITS;
  if (!fmt) fmt = kTsDefaultFormat;
  memset(prog, 0, sizeof(*prog));
  prog->units = units;
  int in = 0, out = 0, nlit = 0;
  auto literal = [&](char c) -> bool {
    TsItem* last = prog->count ? &prog->items[prog->count - 1] : nullptr;
    if (nlit >= kTsMaxLit) return false;
    if (!last || last->spec != 0 || last->width == 255) {
      if (prog->count >= kTsMaxItems) return false;
      last = &prog->items[prog->count++];
      last->spec = 0;
      last->lit = (uint16_t)nlit;
      last->in_off = in;
      last->out_off = out;
    }
    prog->lit[nlit++] = c;
    ++last->width;
    ++last->out_w;
    ++in;
    ++out;
    return true;
  };
  for (const char* p = fmt; *p; ++p) {
    if (*p != '%') {
      if (!literal(*p)) return TS_ERR_TOO_LONG;
      continue;
    }
    if (!*++p) return TS_ERR_UNFINISHED;
    if (*p == '%') {
      if (!literal('%')) return TS_ERR_TOO_LONG;
      continue;
    }
    const int w = ts_spec_width(*p, units);
    if (w < 0) return TS_ERR_SPECIFIER;
    if (prog->count >= kTsMaxItems) return TS_ERR_TOO_LONG;
    TsItem& it = prog->items[prog->count++];
    it.spec = *p;
    it.width = (uint8_t)w;
    it.out_w = (uint8_t)ts_spec_out_width(*p, w);
    it.in_off = in;
    it.out_off = out;
    in += w;
    out += it.out_w;
  }
  prog->width = out;
  prog->in_len = in;
  return TS_OK;
}

// ---- parse (parse_datetime, datetime.cu:160-330) ----------------------------------------------------------------------
enum { TP_YEAR, TP_MONTH, TP_DAY, TP_HOUR, TP_MINUTE, TP_SECOND, TP_SUBSECOND, TP_TZ_MINUTES, TP_COUNT };

// byte i of the row, NUL past its end (deviation 1)
CSDT_HD uint8_t ts_at(const uint8_t* p, int n, int i) { return i < n ? p[i] : (uint8_t)0; }
CSDT_HD int ts_str2int(const uint8_t* p, int n, int at, int bytes) {
  int v = 0;
  for (int k = 0; k < bytes; ++k) {
    const uint8_t c = ts_at(p, n, at + k);
    if (c < '0' || c > '9') break;
    v = v * 10 + (c - '0');
  }
  return v;
}
CSDT_HD uint8_t ts_upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 'a' + 'A') : c; }

// the fields of a row; false = the row fails
CSDT_HD bool parse_ts_parts(const uint8_t* p, int n, const TsProgram& prog, int* tp) {
  for (int i = 0; i < prog.count; ++i) {
    const TsItem it = prog.items[i];
    if (it.spec == 0) continue;  // literals: skipped, never checked
    const int at = it.in_off, w = it.width;
    const int remaining = n - at;
    if (remaining >= 0 && remaining < w) return false;
    switch (it.spec) {
      case 'Y': tp[TP_YEAR] = ts_str2int(p, n, at, w); break;
      case 'y': tp[TP_YEAR] = ts_str2int(p, n, at, w) + 1900; break;
      case 'm': tp[TP_MONTH] = ts_str2int(p, n, at, w); break;
      case 'd': case 'j': tp[TP_DAY] = ts_str2int(p, n, at, w); break;
      case 'H': case 'I': tp[TP_HOUR] = ts_str2int(p, n, at, w); break;
      case 'M': tp[TP_MINUTE] = ts_str2int(p, n, at, w); break;
      case 'S': tp[TP_SECOND] = ts_str2int(p, n, at, w); break;
      case 'f': tp[TP_SUBSECOND] = ts_str2int(p, n, at, w); break;
      case 'p':
        if (tp[TP_HOUR] <= 12 && ts_upper(ts_at(p, n, at)) == 'P' && ts_upper(ts_at(p, n, at + 1)) == 'M') tp[TP_HOUR] += 12;
        break;
      case 'z': {
        const int sign = ts_at(p, n, at) == '-' ? -1 : 1;
        tp[TP_TZ_MINUTES] = sign * (ts_str2int(p, n, at + 1, 2) * 60 + ts_str2int(p, n, at + 3, 2));
        break;
      }
      case 'Z':
        if (ts_upper(ts_at(p, n, at)) != 'U' || ts_upper(ts_at(p, n, at + 1)) != 'T' || ts_upper(ts_at(p, n, at + 2)) != 'C') return false;
        break;
      default: return false;  // a A w b B U W
    }
  }
  return true;
}

// timestamp_from_parts (datetime.cu:270-318); the fields are small (at most 9 digits), only the last scaling can overflow
template <int U>
CSDT_HD int64_t ts_from_parts(const int* tp) {
  int year = tp[TP_YEAR];
  if (U == TS_YEARS) return year - 1970;
  const int month = tp[TP_MONTH];
  if (U == TS_MONTHS) return (int64_t)((year - 1970) * 12 + (month - 1));
  const int day = tp[TP_DAY];
  year -= (month <= 2) ? 1 : 0;
  const int era = (year >= 0 ? year : year - 399) / 400;
  const int yoe = year - era * 400;
  const int doy = month == 0 ? day : ((153 * (month + (month > 2 ? -3 : 9)) + 2) / 5 + day - 1);
  const int doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  const int days = era * 146097 + doe - 719468;
  if (U == TS_DAYS) return days;
  const int tz = tp[TP_TZ_MINUTES];
  const int64_t hour = tp[TP_HOUR];
  if (U == TS_HOURS) return days * (int64_t)24 + hour + tz / 60;
  const int64_t minute = tp[TP_MINUTE];
  if (U == TS_MINUTES) return days * (int64_t)1440 + hour * 60 + minute + tz;
  const int64_t ts = days * (int64_t)86400 + hour * 3600 + minute * 60 + tp[TP_SECOND] + (int64_t)tz * 60;
  if (U == TS_SECONDS) return ts;
  const uint64_t scale = U == TS_MS ? 1000ull : U == TS_US ? 1000000ull : 1000000000ull;
  return (int64_t)((uint64_t)ts * scale + (uint64_t)(int64_t)tp[TP_SUBSECOND]);  // (ns beyond 2262 wraps: deviation 2)
}

// the value of a non-null row (an empty row gives 0)
template <int U>
CSDT_HD int64_t parse_ts_row(const uint8_t* p, int n, const TsProgram& prog) {
  if (n <= 0) return 0;
  int tp[TP_COUNT] = {0, 1, 1, 0, 0, 0, 0, 0};
  if (!parse_ts_parts(p, n, prog, tp)) return 0;
  return ts_from_parts<U>(tp);
}

// ---- format (datetime_formatter, datetime.cu:392-640) -----------------------------------------------------------------
CSDT_HD int ts_wrap32(int64_t v) { return (int)(uint32_t)(uint64_t)v; }

// dissect_timestamp (datetime.cu:404-533)
template <int U>
CSDT_HD void dissect_ts(int64_t v, int* tp) {
  tp[TP_HOUR] = tp[TP_MINUTE] = tp[TP_SECOND] = tp[TP_SUBSECOND] = 0;
  if (U == TS_YEARS) {
    tp[TP_YEAR] = (int)((uint32_t)ts_wrap32(v) + 1970u);
    tp[TP_MONTH] = 1;
    tp[TP_DAY] = 1;
    return;
  }
  if (U == TS_MONTHS) {
    tp[TP_YEAR] = ts_wrap32(v / 12 + 1970);
    tp[TP_MONTH] = (int)(v % 12) + 1;
    tp[TP_DAY] = 1;
    return;
  }
  constexpr int64_t per_day = U == TS_DAYS ? 1 : U == TS_HOURS ? 24 : U == TS_MINUTES ? 1440 : U == TS_SECONDS ? 86400
                              : U == TS_MS ? 86400000LL : U == TS_US ? 86400000000LL : 86400000000000LL;
  int days = ts_wrap32(v / per_day);
  days = (int)((uint32_t)days + 719468u);
  const int monthDayOffset[] = {0, 31, 61, 92, 122, 153, 184, 214, 245, 275, 306, 337, 366};
  int year = 400 * (days / 146097);
  days = days % 146097;
  int leapy = days / 36524;
  days = days % 36524;
  if (leapy == 4) {
    days += 36524;
    --leapy;
  }
  year += 100 * leapy;
  year += 4 * (days / 1461);
  days = days % 1461;
  leapy = days / 365;
  days = days % 365;
  if (leapy == 4) {
    days += 365;
    --leapy;
  }
  year += leapy;
  int month = 12;
  for (int i = 0; i < 12; ++i) {
    if (days < monthDayOffset[i + 1]) {
      month = i;
      break;
    }
  }
  const int day = days - monthDayOffset[month] + 1;
  if (month >= 10) ++year;
  tp[TP_YEAR] = year;
  tp[TP_MONTH] = (month + 2) % 12 + 1;
  tp[TP_DAY] = day;
  if (U == TS_DAYS) return;
  if (U == TS_HOURS) {
    tp[TP_HOUR] = (int)(v % 24);
    return;
  }
  if (U == TS_MINUTES) {
    tp[TP_HOUR] = (int)((v / 60) % 24);
    tp[TP_MINUTE] = (int)(v % 60);
    return;
  }
  constexpr int64_t per_s = U == TS_SECONDS ? 1 : U == TS_MS ? 1000 : U == TS_US ? 1000000 : 1000000000;
  tp[TP_HOUR] = (int)((v / (3600 * per_s)) % 24);
  tp[TP_MINUTE] = (int)((v / (60 * per_s)) % 60);
  tp[TP_SECOND] = (int)((v / per_s) % 60);
  if (U != TS_SECONDS) tp[TP_SUBSECOND] = (int)(v % per_s);
}

// int2str (datetime.cu:536-553): the low `len` digits, zero-padded; a value <= 0 prints as zeros
template <class Out>
CSDT_HD void ts_int2str(Out out, int len, int val) {
  uint32_t u = val > 0 ? (uint32_t)val : 0u;
  for (int k = len - 1; k >= 0; --k) {
    out[k] = (char)('0' + u % 10u);
    u /= 10u;
  }
}

// writes the row (prog.width bytes) to `out`; `Out` is a char pointer of any address space
template <int U, class Out>
CSDT_HD void format_ts_row(int64_t value, const TsProgram& prog, Out out) {
  int tp[TP_COUNT];
  dissect_ts<U>(value, tp);
  for (int i = 0; i < prog.count; ++i) {
    const TsItem it = prog.items[i];
    Out o = out + it.out_off;
    switch (it.spec) {
      case 0:
        for (int k = 0; k < it.width; ++k) o[k] = prog.lit[it.lit + k];
        break;
      case 'Y': ts_int2str(o, it.out_w, tp[TP_YEAR]); break;
      case 'y': ts_int2str(o, it.out_w, (int)((uint32_t)tp[TP_YEAR] - 1900u)); break;
      case 'm': ts_int2str(o, it.out_w, tp[TP_MONTH]); break;
      case 'd': case 'j': ts_int2str(o, it.out_w, tp[TP_DAY]); break;
      case 'H': ts_int2str(o, it.out_w, tp[TP_HOUR]); break;
      case 'I': ts_int2str(o, it.out_w, tp[TP_HOUR] % 12); break;
      case 'M': ts_int2str(o, it.out_w, tp[TP_MINUTE]); break;
      case 'S': ts_int2str(o, it.out_w, tp[TP_SECOND]); break;
      case 'f': ts_int2str(o, it.out_w, tp[TP_SUBSECOND]); break;
      case 'p':
        o[0] = tp[TP_HOUR] <= 12 ? 'A' : 'P';
        o[1] = 'M';
        break;
      case 'Z':
        o[0] = 'U';
        o[1] = 'T';
        o[2] = 'C';
        break;
      default: break;  // z, a A w b B U W: nothing
    }
  }
}

// run-time units -> the template (host code: the harness)
template <class F>
inline auto ts_dispatch(int units, F&& f) {
  switch (units) {
    case TS_YEARS: return f(std::integral_constant<int, TS_YEARS>());
    case TS_MONTHS: return f(std::integral_constant<int, TS_MONTHS>());
    case TS_DAYS: return f(std::integral_constant<int, TS_DAYS>());
    case TS_HOURS: return f(std::integral_constant<int, TS_HOURS>());
    case TS_MINUTES: return f(std::integral_constant<int, TS_MINUTES>());
    case TS_SECONDS: return f(std::integral_constant<int, TS_SECONDS>());
    case TS_MS: return f(std::integral_constant<int, TS_MS>());
    case TS_US: return f(std::integral_constant<int, TS_US>());
    default: return f(std::integral_constant<int, TS_NS>());
  }
}

}  // namespace csdt
#endif
