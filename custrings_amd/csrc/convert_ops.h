/* convert_ops.h -- per-row logic of the numeric and boolean conversions to and from string columns
 * (reference members NVStrings::hash / stoi / stol / stof / stod / htoi / ip2int / to_bools and itos / ltos / ftos /
 * dtos / int2ip / create_from_bools, cpp/src/strings/convert.cu:34-256,373-611,739-994, with the per-string parsers of
 * cpp/src/custring.inl:25-230 and cpp/src/custring_view.inl:1601-1670), restated over a row's bytes.
 *
 * Everything is `__host__ __device__` (plain inline for a host compiler) so that the kernels of cs_convert.hip and the
 * CPU harness of tests/test_convert_cpu.py compile the same text.  Every quirk of the reference is kept:
 *  - stol: one leading sign, digits up to the first other byte, multiplication that wraps (done in unsigned 64-bit
 *    arithmetic here, which is what the reference's machine code does); stoi is (int32)stol.
 *  - stod: digits are cut once they pass 0x0FFFFFFFFFFFFF (later integer digits raise the exponent instead); the byte
 *    after 'e' / 'E' is taken as the exponent's sign even when it is a digit (so "1e5" parses as 1.0); an exponent
 *    above 308 gives +-inf, below -308 +0.0 (sign dropped); "NaN" / "Inf" / "-Inf" (the member) and "nan" / "inf" /
 *    "-inf" (the parser) are whole-row matches; stof is (float)stod.
 *  - htoi: any ASCII letter is a digit ('G' = 16, 'z' = 35); other bytes are skipped; the sum wraps.
 *  - ip2int: exactly three '.' in the row; inside a field every byte that is neither a digit nor '.' is skipped;
 *    fields wrap as u32.  (The reference counts its split('.') tokens in character space; for a one-byte delimiter
 *    that is the number of '.' bytes on valid UTF-8 -- the byte-space convention of row_ops.h.)
 *  - ftos / dtos: the reference's normaliser to 10 significant digits, exactly (-0.0 prints as "0.0").
 *
 * Two documented deviations ("Deviations"):
 *  1. stod scales by P[e], the double nearest to 10^e, where the reference multiplies by CUDA's pow(10.0, e): that
 *     value is not correctly rounded and cannot be reproduced off NVIDIA hardware.  The reference's own known answers
 *     all agree with the table except one row ("-122.33644782", one ulp apart).
 *  2. ltos(INT64_MIN) prints "-9223372036854775808"; the reference negates it (undefined behaviour) and prints "-".
 *
 * Floating-point contraction must be off wherever this header is compiled (dissect_value's
 * `remainder = (v - integer) * max_digits; remainder -= decimal` changes digits when fused into an FMA):
 * csrc/Makefile builds cs_convert.hip with -ffp-contract=off, and the pragma below says the same to clang.
 */
#ifndef CS_CONVERT_OPS_H
#define CS_CONVERT_OPS_H
#include <stdint.h>
#include <string.h>

#include "minhash_ops.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CSCONV_HD __host__ __device__ __forceinline__
#define CSCONV_TABLE __device__ __constant__ static const
#else
#define CSCONV_HD static inline
#define CSCONV_TABLE static const
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace csconv {

// P[e + 308] = the double nearest to 10^e, e in [-308, 308] (written by tools/gen_pow10.py from Python's correctly
// rounded float("1e<e>"); hexadecimal literals so every compiler reads the same bits).
CSCONV_TABLE double kPow10[617] = {
// BEGIN tools/gen_pow10.py
    0x0.730d67819e8d2p-1022, 0x1.1fa182c40c60dp-1020, 0x1.6789e3750f791p-1017, 0x1.c16c5c5253575p-1014,
    0x1.18e3b9b374169p-1010, 0x1.5f1ca820511c3p-1007, 0x1.b6e3d22865634p-1004, 0x1.124e63593f5e1p-1000,
    0x1.56e1fc2f8f359p-997, 0x1.ac9a7b3b7302fp-994, 0x1.0be08d0527e1dp-990, 0x1.4ed8b04671da5p-987,
    0x1.a28edc580e50ep-984, 0x1.059949b708f29p-980, 0x1.46ff9c24cb2f3p-977, 0x1.98bf832dfdfb0p-974,
    0x1.feef63f97d79cp-971, 0x1.3f559e7bee6c1p-967, 0x1.8f2b061aea072p-964, 0x1.f2f5c7a1a488ep-961,
    0x1.37d99cc506d59p-957, 0x1.85d003f6488afp-954, 0x1.e74404f3daadbp-951, 0x1.308a831868ac9p-947,
    0x1.7cad23de82d7bp-944, 0x1.dbd86cd6238d9p-941, 0x1.29674405d6388p-937, 0x1.73c115074bc6ap-934,
    0x1.d0b15a491eb84p-931, 0x1.226ed86db3333p-927, 0x1.6b0a8e891ffffp-924, 0x1.c5cd322b67fffp-921,
    0x1.1ba03f5b21000p-917, 0x1.62884f31e93ffp-914, 0x1.bb2a62fe638ffp-911, 0x1.14fa7ddefe3a0p-907,
    0x1.5a391d56bdc87p-904, 0x1.b0c764ac6d3a9p-901, 0x1.0e7c9eebc444ap-897, 0x1.521bc6a6b555cp-894,
    0x1.a6a2b85062ab3p-891, 0x1.0825b3323dab0p-887, 0x1.4a2f1ffecd15cp-884, 0x1.9cbae7fe805b3p-881,
    0x1.01f4d0ff10390p-877, 0x1.4272053ed4474p-874, 0x1.930e868e89591p-871, 0x1.f7d228322baf5p-868,
    0x1.3ae3591f5b4d9p-864, 0x1.899c2f6732210p-861, 0x1.ec033b40fea93p-858, 0x1.338205089f29cp-854,
    0x1.8062864ac6f43p-851, 0x1.e07b27dd78b14p-848, 0x1.2c4cf8ea6b6ecp-844, 0x1.77603725064a8p-841,
    0x1.d53844ee47dd1p-838, 0x1.25432b14ecea3p-834, 0x1.6e93f5da2824cp-831, 0x1.ca38f350b22dfp-828,
    0x1.1e6398126f5cbp-824, 0x1.65fc7e170b33ep-821, 0x1.bf7b9d9cce00dp-818, 0x1.17ad428200c08p-814,
    0x1.5d98932280f0ap-811, 0x1.b4feb7eb212cdp-808, 0x1.111f32f2f4bc0p-804, 0x1.5566ffafb1eb0p-801,
    0x1.aac0bf9b9e65cp-798, 0x1.0ab877c142ffap-794, 0x1.4d6695b193bf8p-791, 0x1.a0c03b1df8af6p-788,
    0x1.047824f2bb6dap-784, 0x1.45962e2f6a490p-781, 0x1.96fbb9bb44db4p-778, 0x1.fcbaa82a16121p-775,
    0x1.3df4a91a4dcb5p-771, 0x1.8d71d360e13e2p-768, 0x1.f0ce4839198dbp-765, 0x1.3680ed23aff89p-761,
    0x1.8421286c9bf6bp-758, 0x1.e5297287c2f45p-755, 0x1.2f39e794d9d8bp-751, 0x1.7b08617a104eep-748,
    0x1.d9ca79d89462ap-745, 0x1.281e8c275cbdap-741, 0x1.72262f3133ed1p-738, 0x1.ceafbafd80e85p-735,
    0x1.212dd4de70913p-731, 0x1.69794a160cb58p-728, 0x1.c3d79c9b8fe2ep-725, 0x1.1a66c1e139eddp-721,
    0x1.6100725988694p-718, 0x1.b9408eefea839p-715, 0x1.13c85955f2923p-711, 0x1.58ba6fab6f36cp-708,
    0x1.aee90b964b047p-705, 0x1.0d51a73deee2dp-701, 0x1.50a6110d6a9b8p-698, 0x1.a4cf9550c5426p-695,
    0x1.0701bd527b498p-691, 0x1.48c22ca71a1bdp-688, 0x1.9af2b7d0e0a2dp-685, 0x1.00d7b2e28c65cp-681,
    0x1.410d9f9b2f7f3p-678, 0x1.91510781fb5f0p-675, 0x1.f5a549627a36cp-672, 0x1.39874ddd8c623p-668,
    0x1.87e92154ef7acp-665, 0x1.e9e369aa2b597p-662, 0x1.322e220a5b17ep-658, 0x1.7eb9aa8cf1ddep-655,
    0x1.de6815302e556p-652, 0x1.2b010d3e1cf56p-648, 0x1.75c1508da432bp-645, 0x1.d331a4b10d3f6p-642,
    0x1.23ff06eea847ap-638, 0x1.6cfec8aa52598p-635, 0x1.c83e7ad4e6efep-632, 0x1.1d270cc51055fp-628,
    0x1.6470cff6546b6p-625, 0x1.bd8d03f3e9864p-622, 0x1.1678227871f3ep-618, 0x1.5c162b168e70ep-615,
    0x1.b31bb5dc320d2p-612, 0x1.0ff151a99f483p-608, 0x1.53eda614071a4p-605, 0x1.a8e90f9908e0dp-602,
    0x1.0991a9bfa58c8p-598, 0x1.4bf6142f8eefap-595, 0x1.9ef3993b72ab8p-592, 0x1.03583fc527ab3p-588,
    0x1.442e4fb671960p-585, 0x1.9539e3a40dfb8p-582, 0x1.fa885c8d117a6p-579, 0x1.3c9539d82aec8p-575,
    0x1.8bba884e35a7ap-572, 0x1.eea92a61c3118p-569, 0x1.3529ba7d19eafp-565, 0x1.8274291c6065bp-562,
    0x1.e3113363787f2p-559, 0x1.2deac01e2b4f7p-555, 0x1.79657025b6235p-552, 0x1.d7becc2f23ac2p-549,
    0x1.26d73f9d764b9p-545, 0x1.708d0f84d3de7p-542, 0x1.ccb0536608d61p-539, 0x1.1fee341fc585dp-535,
    0x1.67e9c127b6e74p-532, 0x1.c1e43171a4a11p-529, 0x1.192e9ee706e4bp-525, 0x1.5f7a46a0c89ddp-522,
    0x1.b758d848fac55p-519, 0x1.1297872d9cbb5p-515, 0x1.573d68f903ea2p-512, 0x1.ad0cc33744e4bp-509,
    0x1.0c27fa028b0efp-505, 0x1.4f31f8832dd2ap-502, 0x1.a2fe76a3f9475p-499, 0x1.05df0a267bcc9p-495,
    0x1.4756ccb01abfbp-492, 0x1.992c7fdc216fap-489, 0x1.ff779fd329cb9p-486, 0x1.3faac3e3fa1f3p-482,
    0x1.8f9574dcf8a70p-479, 0x1.f37ad21436d0cp-476, 0x1.382cc34ca2428p-472, 0x1.8637f41fcad32p-469,
    0x1.e7c5f127bd87ep-466, 0x1.30dbb6b8d674fp-462, 0x1.7d12a4670c123p-459, 0x1.dc574d80cf16bp-456,
    0x1.29b69070816e3p-452, 0x1.7424348ca1c9cp-449, 0x1.d12d41afca3c3p-446, 0x1.22bc490dde65ap-442,
    0x1.6b6b5b5155ff0p-439, 0x1.c6463225ab7ecp-436, 0x1.1bebdf578b2f4p-432, 0x1.62e6d72d6dfb0p-429,
    0x1.bba08cf8c979dp-426, 0x1.1544581b7dec2p-422, 0x1.5a956e225d672p-419, 0x1.b13ac9aaf4c0fp-416,
    0x1.0ec4be0ad8f89p-412, 0x1.5275ed8d8f36cp-409, 0x1.a71368f0f3047p-406, 0x1.086c219697e2cp-402,
    0x1.4a8729fc3ddb7p-399, 0x1.9d28f47b4d525p-396, 0x1.023998cd10537p-392, 0x1.42c7ff0054685p-389,
    0x1.9379fec069826p-386, 0x1.f8587e7083e30p-383, 0x1.3b374f06526dep-379, 0x1.8a0522c7e7095p-376,
    0x1.ec866b79e0cbap-373, 0x1.33d4032c2c7f5p-369, 0x1.80c903f7379f2p-366, 0x1.e0fb44f50586ep-363,
    0x1.2c9d0b1923745p-359, 0x1.77c44ddf6c516p-356, 0x1.d5b561574765bp-353, 0x1.25915cd68c9f9p-349,
    0x1.6ef5b40c2fc77p-346, 0x1.cab3210f3bb95p-343, 0x1.1eaff4a98553dp-339, 0x1.665bf1d3e6a8dp-336,
    0x1.bff2ee48e0530p-333, 0x1.17f7d4ed8c33ep-329, 0x1.5df5ca28ef40dp-326, 0x1.b5733cb32b111p-323,
    0x1.116805effaeaap-319, 0x1.55c2076bf9a55p-316, 0x1.ab328946f80eap-313, 0x1.0aff95cc5b092p-309,
    0x1.4dbf7b3f71cb7p-306, 0x1.a12f5a0f4e3e5p-303, 0x1.04bd984990e6fp-299, 0x1.45ecfe5bf520bp-296,
    0x1.97683df2f268dp-293, 0x1.fd424d6faf031p-290, 0x1.3e497065cd61fp-286, 0x1.8ddbcc7f40ba6p-283,
    0x1.f152bf9f10e90p-280, 0x1.36d3b7c36a91ap-276, 0x1.8488a5b445360p-273, 0x1.e5aacf2156838p-270,
    0x1.2f8ac174d6123p-266, 0x1.7b6d71d20b96cp-263, 0x1.da48ce468e7c7p-260, 0x1.286d80ec190dcp-256,
    0x1.7288e1271f513p-253, 0x1.cf2b1970e7258p-250, 0x1.217aefe690777p-246, 0x1.69d9abe034955p-243,
    0x1.c45016d841baap-240, 0x1.1ab20e472914ap-236, 0x1.615e91d8f359dp-233, 0x1.b9b6364f30304p-230,
    0x1.1411e1f17e1e3p-226, 0x1.59165a6ddda5bp-223, 0x1.af5bf109550f2p-220, 0x1.0d9976a5d5297p-216,
    0x1.50ffd44f4a73dp-213, 0x1.a53fc9631d10dp-210, 0x1.0747ddddf22a8p-206, 0x1.4919d5556eb52p-203,
    0x1.9b604aaaca626p-200, 0x1.011c2eaabe7d8p-196, 0x1.41633a556e1cep-193, 0x1.91bc08eac9a41p-190,
    0x1.f62b0b257c0d2p-187, 0x1.39dae6f76d883p-183, 0x1.8851a0b548ea4p-180, 0x1.ea6608e29b24dp-177,
    0x1.327fc58da0f70p-173, 0x1.7f1fb6f10934cp-170, 0x1.dee7a4ad4b81fp-167, 0x1.2b50c6ec4f313p-163,
    0x1.7624f8a762fd8p-160, 0x1.d3ae36d13bbcep-157, 0x1.244ce242c5561p-153, 0x1.6d601ad376ab9p-150,
    0x1.c8b8218854567p-147, 0x1.1d7314f534b61p-143, 0x1.64cfda3281e39p-140, 0x1.be03d0bf225c7p-137,
    0x1.16c262777579cp-133, 0x1.5c72fb1552d83p-130, 0x1.b38fb9daa78e4p-127, 0x1.1039d428a8b8fp-123,
    0x1.54484932d2e72p-120, 0x1.a95a5b7f87a0fp-117, 0x1.09d8792fb4c49p-113, 0x1.4c4e977ba1f5cp-110,
    0x1.9f623d5a8a733p-107, 0x1.039d665896880p-103, 0x1.4484bfeebc2a0p-100, 0x1.95a5efea6b347p-97,
    0x1.fb0f6be506019p-94, 0x1.3ce9a36f23c10p-90, 0x1.8c240c4aecb14p-87, 0x1.ef2d0f5da7dd9p-84,
    0x1.357c299a88ea7p-80, 0x1.82db34012b251p-77, 0x1.e392010175ee6p-74, 0x1.2e3b40a0e9b4fp-70,
    0x1.79ca10c924223p-67, 0x1.d83c94fb6d2acp-64, 0x1.2725dd1d243acp-60, 0x1.70ef54646d497p-57,
    0x1.cd2b297d889bcp-54, 0x1.203af9ee75616p-50, 0x1.6849b86a12b9bp-47, 0x1.c25c268497682p-44,
    0x1.19799812dea11p-40, 0x1.5fd7fe1796495p-37, 0x1.b7cdfd9d7bdbbp-34, 0x1.12e0be826d695p-30,
    0x1.5798ee2308c3ap-27, 0x1.ad7f29abcaf48p-24, 0x1.0c6f7a0b5ed8dp-20, 0x1.4f8b588e368f1p-17,
    0x1.a36e2eb1c432dp-14, 0x1.0624dd2f1a9fcp-10, 0x1.47ae147ae147bp-7, 0x1.999999999999ap-4,
    0x1.0000000000000p+0, 0x1.4000000000000p+3, 0x1.9000000000000p+6, 0x1.f400000000000p+9,
    0x1.3880000000000p+13, 0x1.86a0000000000p+16, 0x1.e848000000000p+19, 0x1.312d000000000p+23,
    0x1.7d78400000000p+26, 0x1.dcd6500000000p+29, 0x1.2a05f20000000p+33, 0x1.74876e8000000p+36,
    0x1.d1a94a2000000p+39, 0x1.2309ce5400000p+43, 0x1.6bcc41e900000p+46, 0x1.c6bf526340000p+49,
    0x1.1c37937e08000p+53, 0x1.6345785d8a000p+56, 0x1.bc16d674ec800p+59, 0x1.158e460913d00p+63,
    0x1.5af1d78b58c40p+66, 0x1.b1ae4d6e2ef50p+69, 0x1.0f0cf064dd592p+73, 0x1.52d02c7e14af6p+76,
    0x1.a784379d99db4p+79, 0x1.08b2a2c280291p+83, 0x1.4adf4b7320335p+86, 0x1.9d971e4fe8402p+89,
    0x1.027e72f1f1281p+93, 0x1.431e0fae6d721p+96, 0x1.93e5939a08ceap+99, 0x1.f8def8808b024p+102,
    0x1.3b8b5b5056e17p+106, 0x1.8a6e32246c99cp+109, 0x1.ed09bead87c03p+112, 0x1.3426172c74d82p+116,
    0x1.812f9cf7920e3p+119, 0x1.e17b84357691bp+122, 0x1.2ced32a16a1b1p+126, 0x1.78287f49c4a1dp+129,
    0x1.d6329f1c35ca5p+132, 0x1.25dfa371a19e7p+136, 0x1.6f578c4e0a061p+139, 0x1.cb2d6f618c879p+142,
    0x1.1efc659cf7d4cp+146, 0x1.66bb7f0435c9ep+149, 0x1.c06a5ec5433c6p+152, 0x1.18427b3b4a05cp+156,
    0x1.5e531a0a1c873p+159, 0x1.b5e7e08ca3a8fp+162, 0x1.11b0ec57e649ap+166, 0x1.561d276ddfdc0p+169,
    0x1.aba4714957d30p+172, 0x1.0b46c6cdd6e3ep+176, 0x1.4e1878814c9cep+179, 0x1.a19e96a19fc41p+182,
    0x1.05031e2503da9p+186, 0x1.4643e5ae44d13p+189, 0x1.97d4df19d6057p+192, 0x1.fdca16e04b86dp+195,
    0x1.3e9e4e4c2f344p+199, 0x1.8e45e1df3b015p+202, 0x1.f1d75a5709c1bp+205, 0x1.3726987666191p+209,
    0x1.84f03e93ff9f5p+212, 0x1.e62c4e38ff872p+215, 0x1.2fdbb0e39fb47p+219, 0x1.7bd29d1c87a19p+222,
    0x1.dac74463a989fp+225, 0x1.28bc8abe49f64p+229, 0x1.72ebad6ddc73dp+232, 0x1.cfa698c95390cp+235,
    0x1.21c81f7dd43a7p+239, 0x1.6a3a275d49491p+242, 0x1.c4c8b1349b9b5p+245, 0x1.1afd6ec0e1411p+249,
    0x1.61bcca7119916p+252, 0x1.ba2bfd0d5ff5bp+255, 0x1.145b7e285bf99p+259, 0x1.59725db272f7fp+262,
    0x1.afcef51f0fb5fp+265, 0x1.0de1593369d1bp+269, 0x1.5159af8044462p+272, 0x1.a5b01b605557bp+275,
    0x1.078e111c3556dp+279, 0x1.4971956342ac8p+282, 0x1.9bcdfabc1357ap+285, 0x1.0160bcb58c16cp+289,
    0x1.41b8ebe2ef1c7p+292, 0x1.922726dbaae39p+295, 0x1.f6b0f092959c7p+298, 0x1.3a2e965b9d81dp+302,
    0x1.88ba3bf284e24p+305, 0x1.eae8caef261adp+308, 0x1.32d17ed577d0cp+312, 0x1.7f85de8ad5c4fp+315,
    0x1.df67562d8b363p+318, 0x1.2ba095dc7701ep+322, 0x1.7688bb5394c25p+325, 0x1.d42aea2879f2ep+328,
    0x1.249ad2594c37dp+332, 0x1.6dc186ef9f45cp+335, 0x1.c931e8ab87173p+338, 0x1.1dbf316b346e8p+342,
    0x1.652efdc6018a2p+345, 0x1.be7abd3781ecap+348, 0x1.170cb642b133fp+352, 0x1.5ccfe3d35d80ep+355,
    0x1.b403dcc834e12p+358, 0x1.108269fd210cbp+362, 0x1.54a3047c694fep+365, 0x1.a9cbc59b83a3dp+368,
    0x1.0a1f5b8132466p+372, 0x1.4ca732617ed80p+375, 0x1.9fd0fef9de8e0p+378, 0x1.03e29f5c2b18cp+382,
    0x1.44db473335defp+385, 0x1.961219000356bp+388, 0x1.fb969f40042c5p+391, 0x1.3d3e2388029bbp+395,
    0x1.8c8dac6a0342ap+398, 0x1.efb1178484135p+401, 0x1.35ceaeb2d28c1p+405, 0x1.83425a5f872f1p+408,
    0x1.e412f0f768fadp+411, 0x1.2e8bd69aa19ccp+415, 0x1.7a2ecc414a03fp+418, 0x1.d8ba7f519c84fp+421,
    0x1.27748f9301d32p+425, 0x1.7151b377c247ep+428, 0x1.cda62055b2d9ep+431, 0x1.2087d4358fc82p+435,
    0x1.68a9c942f3ba3p+438, 0x1.c2d43b93b0a8cp+441, 0x1.19c4a53c4e697p+445, 0x1.6035ce8b6203dp+448,
    0x1.b843422e3a84dp+451, 0x1.132a095ce4930p+455, 0x1.57f48bb41db7cp+458, 0x1.adf1aea12525bp+461,
    0x1.0cb70d24b7379p+465, 0x1.4fe4d06de5057p+468, 0x1.a3de04895e46dp+471, 0x1.066ac2d5daec4p+475,
    0x1.4805738b51a75p+478, 0x1.9a06d06e26112p+481, 0x1.00444244d7cabp+485, 0x1.405552d60dbd6p+488,
    0x1.906aa78b912ccp+491, 0x1.f485516e7577fp+494, 0x1.38d352e5096afp+498, 0x1.8708279e4bc5bp+501,
    0x1.e8ca3185deb72p+504, 0x1.317e5ef3ab327p+508, 0x1.7dddf6b095ff1p+511, 0x1.dd55745cbb7edp+514,
    0x1.2a5568b9f52f4p+518, 0x1.74eac2e8727b1p+521, 0x1.d22573a28f19dp+524, 0x1.2357684599702p+528,
    0x1.6c2d4256ffcc3p+531, 0x1.c73892ecbfbf4p+534, 0x1.1c835bd3f7d78p+538, 0x1.63a432c8f5cd6p+541,
    0x1.bc8d3f7b3340cp+544, 0x1.15d847ad00087p+548, 0x1.5b4e5998400a9p+551, 0x1.b221effe500d4p+554,
    0x1.0f5535fef2084p+558, 0x1.532a837eae8a5p+561, 0x1.a7f5245e5a2cfp+564, 0x1.08f936baf85c1p+568,
    0x1.4b378469b6732p+571, 0x1.9e056584240fep+574, 0x1.02c35f729689fp+578, 0x1.4374374f3c2c6p+581,
    0x1.945145230b378p+584, 0x1.f965966bce056p+587, 0x1.3bdf7e0360c36p+591, 0x1.8ad75d8438f43p+594,
    0x1.ed8d34e547314p+597, 0x1.3478410f4c7ecp+601, 0x1.819651531f9e8p+604, 0x1.e1fbe5a7e7861p+607,
    0x1.2d3d6f88f0b3dp+611, 0x1.788ccb6b2ce0cp+614, 0x1.d6affe45f818fp+617, 0x1.262dfeebbb0f9p+621,
    0x1.6fb97ea6a9d38p+624, 0x1.cba7de5054486p+627, 0x1.1f48eaf234ad4p+631, 0x1.671b25aec1d89p+634,
    0x1.c0e1ef1a724ebp+637, 0x1.188d357087713p+641, 0x1.5eb082cca94d7p+644, 0x1.b65ca37fd3a0dp+647,
    0x1.11f9e62fe4448p+651, 0x1.56785fbbdd55ap+654, 0x1.ac1677aad4ab1p+657, 0x1.0b8e0acac4eafp+661,
    0x1.4e718d7d7625ap+664, 0x1.a20df0dcd3af1p+667, 0x1.0548b68a044d6p+671, 0x1.469ae42c8560cp+674,
    0x1.98419d37a6b8fp+677, 0x1.fe52048590673p+680, 0x1.3ef342d37a408p+684, 0x1.8eb0138858d0ap+687,
    0x1.f25c186a6f04cp+690, 0x1.37798f4285630p+694, 0x1.8557f31326bbbp+697, 0x1.e6adefd7f06aap+700,
    0x1.302cb5e6f642ap+704, 0x1.7c37e360b3d35p+707, 0x1.db45dc38e0c82p+710, 0x1.290ba9a38c7d1p+714,
    0x1.734e940c6f9c6p+717, 0x1.d022390f8b837p+720, 0x1.221563a9b7323p+724, 0x1.6a9abc9424febp+727,
    0x1.c5416bb92e3e6p+730, 0x1.1b48e353bce70p+734, 0x1.621b1c28ac20cp+737, 0x1.baa1e332d728fp+740,
    0x1.14a52dffc6799p+744, 0x1.59ce797fb817fp+747, 0x1.b04217dfa61dfp+750, 0x1.0e294eebc7d2cp+754,
    0x1.51b3a2a6b9c76p+757, 0x1.a6208b5068394p+760, 0x1.07d457124123dp+764, 0x1.49c96cd6d16ccp+767,
    0x1.9c3bc80c85c7fp+770, 0x1.01a55d07d39cfp+774, 0x1.420eb449c8843p+777, 0x1.9292615c3aa54p+780,
    0x1.f736f9b3494e9p+783, 0x1.3a825c100dd11p+787, 0x1.8922f31411456p+790, 0x1.eb6bafd91596bp+793,
    0x1.33234de7ad7e3p+797, 0x1.7fec216198ddcp+800, 0x1.dfe729b9ff153p+803, 0x1.2bf07a143f6d4p+807,
    0x1.76ec98994f489p+810, 0x1.d4a7bebfa31abp+813, 0x1.24e8d737c5f0bp+817, 0x1.6e230d05b76cdp+820,
    0x1.c9abd04725481p+823, 0x1.1e0b622c774d0p+827, 0x1.658e3ab795204p+830, 0x1.bef1c9657a686p+833,
    0x1.17571ddf6c814p+837, 0x1.5d2ce55747a18p+840, 0x1.b4781ead1989ep+843, 0x1.10cb132c2ff63p+847,
    0x1.54fdd7f73bf3cp+850, 0x1.aa3d4df50af0bp+853, 0x1.0a6650b926d67p+857, 0x1.4cffe4e7708c0p+860,
    0x1.a03fde214caf1p+863, 0x1.0427ead4cfed6p+867, 0x1.4531e58a03e8cp+870, 0x1.967e5eec84e2fp+873,
    0x1.fc1df6a7a61bbp+876, 0x1.3d92ba28c7d15p+880, 0x1.8cf768b2f9c5ap+883, 0x1.f03542dfb8370p+886,
    0x1.362149cbd3226p+890, 0x1.83a99c3ec7eb0p+893, 0x1.e494034e79e5cp+896, 0x1.2edc82110c2f9p+900,
    0x1.7a93a2954f3b8p+903, 0x1.d9388b3aa30a5p+906, 0x1.27c35704a5e67p+910, 0x1.71b42cc5cf601p+913,
    0x1.ce2137f743382p+916, 0x1.20d4c2fa8a031p+920, 0x1.6909f3b92c83dp+923, 0x1.c34c70a777a4dp+926,
    0x1.1a0fc668aac70p+930, 0x1.6093b802d578cp+933, 0x1.b8b8a6038ad6fp+936, 0x1.137367c236c65p+940,
    0x1.585041b2c477fp+943, 0x1.ae64521f7595ep+946, 0x1.0cfeb353a97dbp+950, 0x1.503e602893dd2p+953,
    0x1.a44df832b8d46p+956, 0x1.06b0bb1fb384cp+960, 0x1.485ce9e7a065fp+963, 0x1.9a742461887f6p+966,
    0x1.008896bcf54fap+970, 0x1.40aabc6c32a38p+973, 0x1.90d56b873f4c7p+976, 0x1.f50ac6690f1f8p+979,
    0x1.3926bc01a973bp+983, 0x1.87706b0213d0ap+986, 0x1.e94c85c298c4cp+989, 0x1.31cfd3999f7b0p+993,
    0x1.7e43c8800759cp+996, 0x1.ddd4baa009303p+999, 0x1.2aa4f4a405be2p+1003, 0x1.754e31cd072dap+1006,
    0x1.d2a1be4048f90p+1009, 0x1.23a516e82d9bap+1013, 0x1.6c8e5ca239029p+1016, 0x1.c7b1f3cac7433p+1019,
    0x1.1ccf385ebc8a0p+1023,
// END tools/gen_pow10.py
};

CSCONV_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
// custr::compare(...) == 0: the same bytes and the same length
CSCONV_HD bool row_equals(const uint8_t* p, int n, const char* s, int m) {
  if (n != m) return false;
  for (int i = 0; i < n; ++i)
    if (p[i] != (uint8_t)s[i]) return false;
  return true;
}

// ---- hash: MurmurHash3_x86_32, seed 31 (custring.inl:164-230); the function itself is minhash_ops.h's, seed as a parameter ----
CSCONV_HD uint32_t hash_row(const uint8_t* p, int n) { return csmh::murmur3_32(p, n, 31u); }

// ---- stol / stoi (custring.inl:25-52) ----------------------------------------------------------------------------------
CSCONV_HD int64_t stol_row(const uint8_t* p, int n) {
  if (n <= 0) return 0;
  int i = 0;
  bool neg = false;
  if (p[0] == '-' || p[0] == '+') {
    neg = p[0] == '-';
    i = 1;
  }
  uint64_t v = 0;
  for (; i < n && is_digit(p[i]); ++i) v = v * 10u + (uint64_t)(p[i] - '0');
  return (int64_t)(neg ? 0u - v : v);
}
CSCONV_HD int32_t stoi_row(const uint8_t* p, int n) { return (int32_t)(uint32_t)(uint64_t)stol_row(p, n); }

// ---- stod / stof (convert.cu:123-190 member checks; custring.inl:70-160 parser) -----------------------------------------
CSCONV_HD double qnan_d() {
  uint64_t b = 0x7FF8000000000000ull;
  double d;
  memcpy(&d, &b, 8);
  return d;
}
CSCONV_HD double inf_d() {
  uint64_t b = 0x7FF0000000000000ull;
  double d;
  memcpy(&d, &b, 8);
  return d;
}
CSCONV_HD double stod_row(const uint8_t* p, int n) {
  if (row_equals(p, n, "NaN", 3)) return qnan_d();  // the member's checks
  if (row_equals(p, n, "Inf", 3)) return inf_d();
  if (row_equals(p, n, "-Inf", 4)) return -inf_d();
  if (n <= 0) return 0.0;
  if (row_equals(p, n, "nan", 3)) return qnan_d();  // the parser's
  if (row_equals(p, n, "inf", 3)) return inf_d();
  if (row_equals(p, n, "-inf", 4)) return -inf_d();
  int i = 0;
  double sign = 1.0;
  if (p[0] == '-' || p[0] == '+') {
    sign = p[0] == '-' ? -1.0 : 1.0;
    ++i;
  }
  const uint64_t max_mantissa = 0x0FFFFFFFFFFFFFull;
  uint64_t digits = 0;
  uint32_t exp_off = 0;  // (int arithmetic of the reference, wrapping)
  bool decimal = false;
  for (; i < n; ++i) {
    const uint8_t c = p[i];
    if (c == '.') {
      decimal = true;
      continue;
    }
    if (!is_digit(c)) break;
    if (digits > max_mantissa) {
      exp_off += (uint32_t)!decimal;
    } else {
      digits = digits * 10u + (uint64_t)(c - '0');
      if (digits > max_mantissa) {
        digits /= 10u;
        exp_off += (uint32_t)!decimal;
      } else {
        exp_off -= (uint32_t)decimal;
      }
    }
  }
  uint32_t exp10 = 0, exp_sign = 1;
  if (i < n) {
    uint8_t c = p[i++];
    if (c == 'e' || c == 'E') {
      if (i < n) {
        c = p[i++];  // (taken as the sign even when it is a digit)
        if (c == '-' || c == '+') exp_sign = c == '-' ? 0xFFFFFFFFu : 1u;
        while (i < n) {
          c = p[i++];
          if (!is_digit(c)) break;
          exp10 = exp10 * 10u + (uint32_t)(c - '0');
        }
      }
    }
  }
  const int e = (int)(exp10 * exp_sign + exp_off);
  if (e > 308) return sign > 0 ? inf_d() : -inf_d();
  if (e < -308) return 0.0;
  // DEVIATION 1: the reference multiplies by CUDA's pow(10.0, e), which is not correctly rounded; P[e] is.
  const double value = (double)digits * kPow10[e + 308];
  return value * sign;
}
CSCONV_HD float stof_row(const uint8_t* p, int n) { return (float)stod_row(p, n); }

// ---- htoi (convert.cu:193-240) -----------------------------------------------------------------------------------------
CSCONV_HD uint32_t htoi_row(const uint8_t* p, int n) {
  uint64_t result = 0, base = 1;
  for (int i = n - 1; i >= 0; --i) {
    const uint8_t c = p[i];
    uint64_t d;
    if (c >= '0' && c <= '9') d = c - 48u;
    else if (c >= 'A' && c <= 'Z') d = c - 55u;
    else if (c >= 'a' && c <= 'z') d = c - 87u;
    else continue;
    result += d * base;
    base *= 16u;
  }
  return (uint32_t)result;
}

// ---- ip2int (convert.cu:739-786) ---------------------------------------------------------------------------------------
CSCONV_HD uint32_t ip2int_row(const uint8_t* p, int n) {
  if (n <= 0) return 0;
  int dots = 0;
  for (int i = 0; i < n; ++i) dots += p[i] == '.';
  if (dots != 3) return 0;
  uint32_t v[4] = {0, 0, 0, 0};
  int iv = 0;
  for (int i = 0; i < n && iv < 4; ++i) {
    const uint8_t c = p[i];
    if (is_digit(c)) v[iv] = v[iv] * 10u + (uint32_t)(c - '0');
    else if (c == '.') ++iv;
  }
  return v[0] * 16777216u + v[1] * 65536u + v[2] * 256u + v[3];
}

// ---- to_bools (convert.cu:878-925): null rows are `true_string == nullptr` ----------------------------------------------
CSCONV_HD uint8_t to_bool_row(const uint8_t* p, int n, const uint8_t* t, int tn) {
  if (!t) return 0;
  if (n != tn) return 0;
  for (int i = 0; i < n; ++i)
    if (p[i] != t[i]) return 0;
  return 1;
}

// ---- ltos / itos (custring_view.inl:1626-1670) ---------------------------------------------------------------------------
constexpr int kMaxNumWidth = 20;  // "-9223372036854775808": the widest row of the numeric formats
CSCONV_HD int ltos_row(int64_t value, char* out) {
  if (value == 0) {
    out[0] = '0';
    return 1;
  }
  const bool neg = value < 0;
  // DEVIATION 2: INT64_MIN prints its digits (the reference negates it -- undefined -- and prints "-").
  uint64_t u = neg ? 0u - (uint64_t)value : (uint64_t)value;
  char buf[20];
  int k = 0;
  while (u > 0) {
    buf[k++] = (char)('0' + (int)(u % 10u));
    u /= 10u;
  }
  int len = 0;
  if (neg) out[len++] = '-';
  while (k > 0) out[len++] = buf[--k];
  return len;
}

// ---- int2ip (convert.cu:788-876) -------------------------------------------------------------------------------------
CSCONV_HD int int2ip_row(uint32_t ip, char* out) {
  int len = 0;
  for (int j = 3; j >= 0; --j) {
    const int v = (int)((ip >> (8 * j)) & 255u);
    if (v >= 100) out[len++] = (char)('0' + v / 100);
    if (v >= 10) out[len++] = (char)('0' + (v / 10) % 10);
    out[len++] = (char)('0' + v % 10);
    if (j) out[len++] = '.';
  }
  return len;
}

// ---- ftos / dtos: the reference's ftos_converter (convert.cu:373-548) -----------------------------------------------------
CSCONV_HD int int2str(unsigned value, char* out) {
  if (value == 0) {
    out[0] = '0';
    return 1;
  }
  char buf[10];
  int k = 0;
  while (value > 0) {
    buf[k++] = (char)('0' + value % 10u);
    value /= 10u;
  }
  int len = 0;
  while (k > 0) out[len++] = buf[--k];
  return len;
}
CSCONV_HD int dissect_value(double value, unsigned& integer, unsigned& decimal, int& exp10) {
  const double upper10[9] = {10, 100, 10000, 1e8, 1e16, 1e32, 1e64, 1e128, 1e256};
  const double lower10[9] = {.1, .01, .0001, 1e-8, 1e-16, 1e-32, 1e-64, 1e-128, 1e-256};
  const double blower10[9] = {1.0, .1, .001, 1e-7, 1e-15, 1e-31, 1e-63, 1e-127, 1e-255};
  int decimal_places = 10 - 1;
  exp10 = 0;
  if (value > 1000000000.0) {
    int fx = 256;
    for (int idx = 8; idx >= 0; --idx) {
      if (value >= upper10[idx]) {
        value *= lower10[idx];
        exp10 += fx;
      }
      fx >>= 1;
    }
  } else if (value > 0.0 && value < 0.0001) {
    int fx = 256;
    for (int idx = 8; idx >= 0; --idx) {
      if (value < blower10[idx]) {
        value *= upper10[idx];
        exp10 -= fx;
      }
      fx >>= 1;
    }
  }
  unsigned max_digits = 1000000000u;
  integer = (unsigned)value;
  for (unsigned i = integer; i >= 10; i /= 10) {
    --decimal_places;
    max_digits /= 10;
  }
  double remainder = (value - (double)integer) * (double)max_digits;
  decimal = (unsigned)remainder;
  remainder -= (double)decimal;  // (must not fuse with the product above: contraction off)
  decimal += (unsigned)(2.0 * remainder);
  if (decimal >= max_digits) {
    decimal = 0;
    ++integer;
    if (exp10 && integer >= 10) {
      ++exp10;
      integer = 1;
    }
  }
  while ((decimal % 10) == 0 && decimal_places > 0) {
    decimal /= 10;
    --decimal_places;
  }
  return decimal_places;
}
// at most kMaxNumWidth bytes
CSCONV_HD int dtos_row(double value, char* out) {
  if (value != value) {
    out[0] = 'N', out[1] = 'a', out[2] = 'N';
    return 3;
  }
  bool neg = false;
  if (value < 0.0) {
    value = -value;
    neg = true;
  }
  if (value == inf_d()) {
    int len = 0;
    if (neg) out[len++] = '-';
    out[len++] = 'I', out[len++] = 'n', out[len++] = 'f';
    return len;
  }
  unsigned integer = 0, decimal = 0;
  int exp10 = 0;
  int places = dissect_value(value, integer, decimal, exp10);
  int len = 0;
  if (neg) out[len++] = '-';
  len += int2str(integer, out + len);
  out[len++] = '.';
  if (places) {
    for (int k = places - 1; k >= 0; --k) {
      out[len + k] = (char)('0' + decimal % 10u);
      decimal /= 10u;
    }
    len += places;
  } else {
    out[len++] = '0';
  }
  if (exp10) {
    out[len++] = 'e';
    if (exp10 < 0) {
      out[len++] = '-';
      exp10 = -exp10;
    } else {
      out[len++] = '+';
    }
    if (exp10 < 10) out[len++] = '0';
    len += int2str((unsigned)exp10, out + len);
  }
  return len;
}
CSCONV_HD int ftos_row(float value, char* out) { return dtos_row((double)value, out); }

}  // namespace csconv

#endif
