// pybind11 bindings of the HIP kernel library + native executor (module kdl._C).
// Device pointers and hipStream_t travel as Python ints (torch: .data_ptr(),
// torch.cuda.current_stream().cuda_stream); no torch headers are needed, which
// keeps the extension a plain hipcc build (no hipify, no CUDA shims).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "kernels/launch.h"
#include "runtime/jpeg_huff.h"
#include "runtime/engine.h"
#include "runtime/comm.h"
#include "runtime/dp_hiploop.h"
#include "runtime/hip_backend.h"

namespace py = pybind11;
using namespace kdl;

namespace {

template <typename T>
T* P(const py::dict& d, const char* k) {
  if (!d.contains(k) || d[k].is_none()) return nullptr;
  return reinterpret_cast<T*>(d[k].cast<uintptr_t>());
}
int I(const py::dict& d, const char* k, int def = 0) {
  if (!d.contains(k) || d[k].is_none()) return def;
  return d[k].cast<int>();
}
hipStream_t S(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

ConvGemmArgs conv_args(const py::dict& d) {
  ConvGemmArgs a{};
  a.x = P<const uint16_t>(d, "x");
  a.wp = P<const uint16_t>(d, "wp");
  a.bias = P<const float>(d, "bias");
  a.dww = P<const float>(d, "dww");
  a.dwk = P<const uint16_t>(d, "dwk");
  a.res = P<const uint16_t>(d, "res");
  a.y = P<uint16_t>(d, "y");
  a.stamps = P<unsigned long long>(d, "stamps");
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W");
  a.OH = I(d, "OH"); a.OW = I(d, "OW"); a.M = I(d, "M");
  a.ldx = I(d, "ldx"); a.ldy = I(d, "ldy"); a.ldr = I(d, "ldr");
  a.K = I(d, "K"); a.cin = I(d, "cin", 32); a.NF = I(d, "NF");
  a.nstore = I(d, "nstore"); a.stride = I(d, "stride", 1);
  a.relu_in = I(d, "relu_in"); a.relu_out = I(d, "relu_out"); a.opad = I(d, "opad");
  a.dt = I(d, "dt");
  a.krot = I(d, "krot");
  a.ksplit = I(d, "ksplit");
  a.ws = P<float>(d, "ws");
  a.cnt = P<int>(d, "cnt");
  a.ascale = P<const float>(d, "ascale");
  a.ascale_ld = I(d, "ascale_ld");
  return a;
}
float F(const py::dict& d, const char* k, float def) {
  if (!d.contains(k) || d[k].is_none()) return def;
  return d[k].cast<float>();
}
StemArgs stem_args(const py::dict& d) {
  StemArgs a{};
  a.x = P<const void>(d, "x"); a.wp = P<const uint16_t>(d, "wp");
  a.bias = P<const float>(d, "bias"); a.y = P<uint16_t>(d, "y");
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W");
  a.OH = I(d, "OH"); a.OW = I(d, "OW"); a.ldy = I(d, "ldy"); a.in_kind = I(d, "in_kind");
  // defaults = the Xception stem (3x3 s2 'valid' -> 32, normalisation folded into the weights)
  a.KH = I(d, "KH", 3); a.KW = I(d, "KW", 3); a.stride = I(d, "stride", 2); a.pad = I(d, "pad", 0);
  a.cout = I(d, "cout", 32); a.relu = I(d, "relu", 1); a.dt = I(d, "dt");
  const char* sk[3] = {"scale0", "scale1", "scale2"};
  const char* hk[3] = {"shift0", "shift1", "shift2"};
  for (int c = 0; c < 3; ++c) { a.scale[c] = F(d, sk[c], 1.f); a.shift[c] = F(d, hk[c], 0.f); }
  a.rows = I(d, "rows", 0);
  return a;
}
StemConvArgs stem_conv_args(const py::dict& d) {
  StemConvArgs a{};
  a.x = P<const uint8_t>(d, "x"); a.wp1 = P<const uint16_t>(d, "wp1"); a.b1 = P<const float>(d, "b1");
  a.wp2 = P<const uint16_t>(d, "wp2"); a.b2 = P<const float>(d, "b2"); a.y = P<uint16_t>(d, "y");
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W"); a.H1 = I(d, "H1"); a.W1 = I(d, "W1");
  a.OH = I(d, "OH"); a.OW = I(d, "OW"); a.ldy = I(d, "ldy"); a.NF = I(d, "NF"); a.nstore = I(d, "nstore");
  a.relu_out = I(d, "relu_out"); a.grid = I(d, "grid");
  return a;
}
GapArgs gap_args(const py::dict& d) {
  GapArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.y = P<float>(d, "y"); a.yb = P<uint16_t>(d, "yb");
  a.B = I(d, "B"); a.HW = I(d, "HW"); a.ldx = I(d, "ldx"); a.F = I(d, "F"); a.dt = I(d, "dt");
  return a;
}
FcArgs fc_args(const py::dict& d) {
  FcArgs a{};
  a.x = P<const float>(d, "x"); a.w = P<const float>(d, "w"); a.bias = P<const float>(d, "bias");
  a.out = P<float>(d, "out");
  a.B = I(d, "B"); a.F = I(d, "F"); a.N = I(d, "N"); a.relu = I(d, "relu");
  return a;
}
PatchifyArgs patch_args(const py::dict& d) {
  PatchifyArgs a{};
  a.x = P<const uint8_t>(d, "x"); a.y = P<uint16_t>(d, "y");
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W"); a.P = I(d, "P"); a.ldy = I(d, "ldy");
  const char* sk[3] = {"scale0", "scale1", "scale2"};
  const char* hk[3] = {"shift0", "shift1", "shift2"};
  for (int c = 0; c < 3; ++c) { a.scale[c] = F(d, sk[c], 1.f); a.shift[c] = F(d, hk[c], 0.f); }
  return a;
}
EmbedArgs embed_args(const py::dict& d) {
  EmbedArgs a{};
  a.x = P<uint16_t>(d, "x"); a.cls = P<const float>(d, "cls"); a.pos = P<const float>(d, "pos");
  a.B = I(d, "B"); a.T = I(d, "T"); a.D = I(d, "D");
  return a;
}
LnArgs ln_args(const py::dict& d) {
  LnArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.y = P<uint16_t>(d, "y");
  a.gamma = P<const float>(d, "gamma"); a.beta = P<const float>(d, "beta");
  a.y8 = P<uint8_t>(d, "y8"); a.inv_scale = F(d, "inv_scale", 1.f);
  a.rows = d["rows"].cast<long>(); a.D = I(d, "D"); a.ldx = I(d, "ldx"); a.ldy = I(d, "ldy");
  a.eps = F(d, "eps", 1e-6f);
  return a;
}
AttnArgs attn_args(const py::dict& d) {
  AttnArgs a{};
  a.qkv = P<const uint16_t>(d, "qkv"); a.out = P<uint16_t>(d, "out");
  a.out8 = P<uint8_t>(d, "out8"); a.inv_scale = F(d, "inv_scale", 1.f);
  a.B = I(d, "B"); a.T = I(d, "T"); a.H = I(d, "H"); a.dh = I(d, "dh", 64);
  a.scale = F(d, "scale", 0.125f); a.algo = I(d, "algo", 0);
  return a;
}
DwkArgs dwk_args(const py::dict& d) {
  DwkArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.w = P<const float>(d, "w"); a.bias = P<const float>(d, "bias");
  a.y = P<uint16_t>(d, "y"); a.pool = P<float>(d, "pool"); a.w1 = P<const float>(d, "w1");
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W"); a.C = I(d, "C"); a.OH = I(d, "OH"); a.OW = I(d, "OW");
  a.K = I(d, "K"); a.S = I(d, "S", 1); a.pad = I(d, "pad"); a.act = I(d, "act"); a.Cs = I(d, "Cs");
  a.cg = I(d, "cg", 0); a.rb = I(d, "rb", 0); a.tw = I(d, "tw", 0); a.seg = I(d, "seg", 0);
  a.lds_kb = I(d, "lds_kb", 0); a.algo = I(d, "algo", 0); a.pd = I(d, "pd", 0);
  return a;
}
SeArgs se_args(const py::dict& d) {
  SeArgs a{};
  a.pool = P<const float>(d, "pool"); a.b1 = P<const float>(d, "b1");
  a.w2t = P<const float>(d, "w2t"); a.b2 = P<const float>(d, "b2"); a.scale = P<float>(d, "scale");
  a.B = I(d, "B"); a.ntiles = I(d, "ntiles"); a.HW = I(d, "HW"); a.C = I(d, "C"); a.Cs = I(d, "Cs");
  return a;
}
ChScaleArgs chs_args(const py::dict& d) {
  ChScaleArgs a{};
  a.y = P<uint16_t>(d, "y"); a.scale = P<const float>(d, "scale");
  a.B = I(d, "B"); a.HW = I(d, "HW"); a.C = I(d, "C");
  return a;
}
GemmF8Args f8_args(const py::dict& d) {
  GemmF8Args a{};
  a.x = P<const uint8_t>(d, "x"); a.wp = P<const uint8_t>(d, "wp"); a.bias = P<const float>(d, "bias");
  a.colscale = P<const float>(d, "colscale"); a.res = P<const uint16_t>(d, "res");
  a.y = P<uint16_t>(d, "y"); a.y8 = P<uint8_t>(d, "y8"); a.out_inv_scale = F(d, "out_inv_scale", 1.f);
  a.M = I(d, "M"); a.K = I(d, "K"); a.ldx = I(d, "ldx"); a.ldy = I(d, "ldy"); a.ldr = I(d, "ldr");
  a.NF = I(d, "NF"); a.nstore = I(d, "nstore"); a.relu_out = I(d, "relu_out");
  a.krot = I(d, "krot");
  return a;
}
EntryBlockArgs eb_args(const py::dict& d) {
  EntryBlockArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.y = P<uint16_t>(d, "y");
  a.w1 = P<const uint16_t>(d, "w1"); a.b1 = P<const float>(d, "b1"); a.dw1 = P<const float>(d, "dw1");
  a.w2 = P<const uint16_t>(d, "w2"); a.b2 = P<const float>(d, "b2"); a.dw2 = P<const float>(d, "dw2");
  a.dwk1 = P<const uint16_t>(d, "dwk1"); a.dwk2 = P<const uint16_t>(d, "dwk2");
  a.wr = P<const uint16_t>(d, "wr"); a.br = P<const float>(d, "br");
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W"); a.OH = I(d, "OH"); a.OW = I(d, "OW");
  a.ldx = I(d, "ldx"); a.ldy = I(d, "ldy"); a.grid = I(d, "grid");
  a.steps = P<const int4>(d, "steps"); a.step_off = P<const int>(d, "step_off");
  a.stamps = P<unsigned long long>(d, "stamps");
  if (!a.x || !a.y || !a.w1 || !a.b1 || !a.dw1 || !a.w2 || !a.b2 || !a.dw2 || !a.wr || !a.br)
    throw std::invalid_argument("entry_block: null pointer");
  return a;
}

FcMfmaArgs fcm_args(const py::dict& d) {
  FcMfmaArgs a{};
  a.xb = P<const uint16_t>(d, "xb"); a.wp = P<const uint16_t>(d, "wp"); a.bias = P<const float>(d, "bias");
  a.out = P<float>(d, "out");
  a.B = I(d, "B"); a.F = I(d, "F"); a.N = I(d, "N"); a.NF = I(d, "NF"); a.relu = I(d, "relu");
  a.dt = I(d, "dt");
  return a;
}
PoolAddArgs pool_args(const py::dict& d) {
  PoolAddArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.res = P<const uint16_t>(d, "res"); a.y = P<uint16_t>(d, "y");
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W"); a.OH = I(d, "OH"); a.OW = I(d, "OW");
  a.C = I(d, "C"); a.pad_top = I(d, "pad_top"); a.pad_left = I(d, "pad_left"); a.dt = I(d, "dt");
  a.algo = d.contains("algo") ? I(d, "algo") : 0;
  a.seg = d.contains("seg") ? I(d, "seg") : 0; a.rb = d.contains("rb") ? I(d, "rb") : 0;
  return a;
}
HeadArgs head_args(const py::dict& d) {
  HeadArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.w1 = P<const float>(d, "w1"); a.b1 = P<const float>(d, "b1");
  a.w2 = P<const float>(d, "w2"); a.b2 = P<const float>(d, "b2"); a.out = P<float>(d, "out");
  a.feat = P<float>(d, "feat"); a.hid = P<float>(d, "hid");
  a.B = I(d, "B"); a.HW = I(d, "HW"); a.ldx = I(d, "ldx"); a.F = I(d, "F"); a.H1 = I(d, "H1");
  a.NC = I(d, "NC");
  return a;
}
TopkArgs topk_args(const py::dict& d) {
  TopkArgs a{};
  a.x = P<const float>(d, "x"); a.out = P<int32_t>(d, "out");
  a.B = I(d, "B"); a.NC = I(d, "NC"); a.K = I(d, "K"); a.ldx = I(d, "ldx");
  return a;
}
EmbedRowsArgs embed_rows_args(const py::dict& d) {
  EmbedRowsArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.out = P<float>(d, "out");
  a.B = I(d, "B"); a.HW = I(d, "HW"); a.F = I(d, "F"); a.ldx = I(d, "ldx"); a.ldo = I(d, "ldo");
  a.dt = I(d, "dt"); a.norm = I(d, "norm");
  return a;
}
GalleryTopkArgs gallery_topk_args(const py::dict& d) {
  GalleryTopkArgs a{};
  a.q = P<const float>(d, "q"); a.g = P<const uint16_t>(d, "g"); a.out = P<int32_t>(d, "out");
  a.work = P<void>(d, "work");
  a.B = I(d, "B"); a.N = I(d, "N"); a.F = I(d, "F"); a.K = I(d, "K"); a.ldq = I(d, "ldq"); a.ldg = I(d, "ldg");
  return a;
}
ClassMapArgs class_map_args(const py::dict& d) {
  ClassMapArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.top = P<const int32_t>(d, "top"); a.w = P<const uint16_t>(d, "w");
  a.w1 = P<const float>(d, "w1"); a.w2 = P<const float>(d, "w2"); a.b1 = P<const float>(d, "b1");
  a.hid = P<const float>(d, "hid"); a.alpha = P<float>(d, "alpha"); a.out = P<float>(d, "out");
  a.B = I(d, "B"); a.HW = I(d, "HW"); a.F = I(d, "F"); a.ldx = I(d, "ldx"); a.ldo = I(d, "ldo");
  a.NC = I(d, "NC"); a.H1 = I(d, "H1"); a.dt = I(d, "dt"); a.head = I(d, "head"); a.norm = I(d, "norm");
  return a;
}
AttnRolloutArgs attn_rollout_args(const py::dict& d) {
  AttnRolloutArgs a{};
  a.qkv = P<const uint16_t>(d, "qkv"); a.r_in = P<const float>(d, "r_in"); a.r_out = P<float>(d, "r_out");
  a.B = I(d, "B"); a.T = I(d, "T"); a.Tq = I(d, "Tq"); a.H = I(d, "H"); a.dh = I(d, "dh", 64);
  a.scale = F(d, "scale", 0.125f); a.ldr = I(d, "ldr");
  return a;
}
RolloutMapArgs rollout_map_args(const py::dict& d) {
  RolloutMapArgs a{};
  a.r = P<const float>(d, "r"); a.top = P<const int32_t>(d, "top"); a.out = P<float>(d, "out");
  a.B = I(d, "B"); a.T = I(d, "T"); a.ldr = I(d, "ldr"); a.ldo = I(d, "ldo");
  return a;
}
HeatOverlayArgs heat_overlay_args(const py::dict& d) {
  HeatOverlayArgs a{};
  a.inp = P<const uint8_t>(d, "inp"); a.out = P<float>(d, "out"); a.tab = P<const uint8_t>(d, "tab");
  a.xb = P<const int32_t>(d, "xb"); a.xk = P<const int32_t>(d, "xk"); a.yb = P<const int32_t>(d, "yb");
  a.yk = P<const int32_t>(d, "yk"); a.h_xb = P<const int32_t>(d, "h_xb"); a.h_yb = P<const int32_t>(d, "h_yb");
  a.B = I(d, "B"); a.S = I(d, "S"); a.h = I(d, "h"); a.w = I(d, "w"); a.ldo = I(d, "ldo");
  a.xks = I(d, "xks"); a.yks = I(d, "yks"); a.a = I(d, "a"); a.blend = I(d, "blend");
  return a;
}
PaletteArgs palette_args(const py::dict& d) {
  PaletteArgs a{};
  a.inp = P<const uint8_t>(d, "inp"); a.out = P<float>(d, "out"); a.work = P<uint32_t>(d, "work");
  a.xb = P<const int32_t>(d, "xb"); a.xk = P<const int32_t>(d, "xk"); a.yb = P<const int32_t>(d, "yb");
  a.yk = P<const int32_t>(d, "yk"); a.h_xb = P<const int32_t>(d, "h_xb"); a.h_yb = P<const int32_t>(d, "h_yb");
  a.B = I(d, "B"); a.S = I(d, "S"); a.h = I(d, "h"); a.w = I(d, "w"); a.ldo = I(d, "ldo");
  a.xks = I(d, "xks"); a.yks = I(d, "yks"); a.K = I(d, "K"); a.T = I(d, "T"); a.weight = I(d, "weight", -1);
  return a;
}
LocateArgs locate_args(const py::dict& d) {
  LocateArgs a{};
  a.out = P<float>(d, "out"); a.work = P<uint8_t>(d, "work");
  a.xb = P<const int32_t>(d, "xb"); a.xk = P<const int32_t>(d, "xk"); a.yb = P<const int32_t>(d, "yb");
  a.yk = P<const int32_t>(d, "yk"); a.h_xb = P<const int32_t>(d, "h_xb"); a.h_yb = P<const int32_t>(d, "h_yb");
  a.B = I(d, "B"); a.S = I(d, "S"); a.h = I(d, "h"); a.w = I(d, "w"); a.ldo = I(d, "ldo");
  a.xks = I(d, "xks"); a.yks = I(d, "yks"); a.K = I(d, "K"); a.threshold = I(d, "threshold");
  return a;
}
CutoutArgs cutout_args(const py::dict& d) {
  CutoutArgs a{};
  a.inp = P<const uint8_t>(d, "inp"); a.out = P<float>(d, "out"); a.work = P<uint8_t>(d, "work");
  a.xb = P<const int32_t>(d, "xb"); a.xk = P<const int32_t>(d, "xk"); a.yb = P<const int32_t>(d, "yb");
  a.yk = P<const int32_t>(d, "yk"); a.h_xb = P<const int32_t>(d, "h_xb"); a.h_yb = P<const int32_t>(d, "h_yb");
  a.B = I(d, "B"); a.S = I(d, "S"); a.h = I(d, "h"); a.w = I(d, "w"); a.ldo = I(d, "ldo");
  a.xks = I(d, "xks"); a.yks = I(d, "yks"); a.gate = I(d, "gate"); a.rounds = I(d, "rounds", -1);
  a.smooth = I(d, "smooth", -1); a.feather = I(d, "feather", -1);
  return a;
}
JpegEncodeArgs jpeg_encode_args(const py::dict& d) {
  JpegEncodeArgs a{};
  a.inp = P<const uint8_t>(d, "inp"); a.hdr = P<const uint8_t>(d, "hdr"); a.h_hdr = P<const uint8_t>(d, "h_hdr");
  a.front = P<const uint32_t>(d, "front"); a.out = P<uint32_t>(d, "out"); a.work = P<void>(d, "work");
  a.ldi = (d.contains("ldi") && !d["ldi"].is_none()) ? d["ldi"].cast<int64_t>() : 0;
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W"); a.quality = I(d, "quality"); a.sampling = I(d, "sampling", -1);
  a.cap = I(d, "cap"); a.ldo = I(d, "ldo"); a.nfront = I(d, "nfront"); a.ldf = I(d, "ldf");
  return a;
}
ResizeArgs resize_args(const py::dict& d) {
  ResizeArgs a{};
  a.src = P<const uint8_t>(d, "src"); a.dst = P<uint8_t>(d, "dst");
  a.ytab = P<const int>(d, "ytab"); a.xtab = P<const int>(d, "xtab");
  a.SH = I(d, "SH"); a.SW = I(d, "SW"); a.OH = I(d, "OH"); a.OW = I(d, "OW"); a.n = I(d, "n", 1);
  return a;
}

JpegArgs jpeg_args(const py::dict& d) {
  JpegArgs a{};
  a.desc = P<const JpegDesc>(d, "desc"); a.h_desc = P<const JpegDesc>(d, "h_desc");
  a.coef = P<const int16_t>(d, "coef"); a.qt = P<const uint16_t>(d, "qt");
  a.planes = P<uint8_t>(d, "planes"); a.out = P<uint8_t>(d, "out");
  a.coef_cap = d["coef_cap"].cast<uint64_t>(); a.plane_cap = d["plane_cap"].cast<uint64_t>();
  a.qt_cap = I(d, "qt_cap"); a.n = I(d, "n"); a.n_wg = I(d, "n_wg"); a.out_rows = I(d, "out_rows");
  a.OH = I(d, "OH"); a.OW = I(d, "OW");
  return a;
}

uint64_t U64(const py::dict& d, const char* k) {
  if (!d.contains(k) || d[k].is_none()) return 0;
  return d[k].cast<uint64_t>();
}
JpegHuffArgs jpeg_huff_args(const py::dict& d) {
  JpegHuffArgs a{};
  a.desc = P<const JpegHuffDesc>(d, "desc"); a.h_desc = P<const JpegHuffDesc>(d, "h_desc");
  a.stage = P<const uint8_t>(d, "stage"); a.coef = P<int16_t>(d, "coef"); a.status = P<uint32_t>(d, "status");
  a.stage_cap = U64(d, "stage_cap"); a.coef_cap = U64(d, "coef_cap");
  a.status_cap = I(d, "status_cap"); a.n = I(d, "n");
  a.h_stage = P<const uint8_t>(d, "h_stage");
  return a;
}
ResampleArgs resample_args(const py::dict& d) {
  ResampleArgs a{};
  a.desc = P<const ResampleDesc>(d, "desc"); a.h_desc = P<const ResampleDesc>(d, "h_desc");
  a.jdesc = P<const JpegDesc>(d, "jdesc"); a.h_jdesc = P<const JpegDesc>(d, "h_jdesc");
  a.planes = P<const uint8_t>(d, "planes"); a.tmp = P<uint8_t>(d, "tmp"); a.out = P<uint8_t>(d, "out");
  a.plane_cap = U64(d, "plane_cap"); a.tmp_cap = U64(d, "tmp_cap");
  a.n_jdesc = I(d, "n_jdesc"); a.n = I(d, "n"); a.out_rows = I(d, "out_rows");
  a.OH = I(d, "OH"); a.OW = I(d, "OW");
  return a;
}

DwArgs dw_args(const py::dict& d) {
  DwArgs a{};
  a.x = P<const uint16_t>(d, "x"); a.w = P<const float>(d, "w"); a.y = P<uint16_t>(d, "y");
  a.B = I(d, "B"); a.H = I(d, "H"); a.W = I(d, "W"); a.C = I(d, "C"); a.relu_in = I(d, "relu_in");
  a.cg = d.contains("cg") ? I(d, "cg") : 0; a.rb = d.contains("rb") ? I(d, "rb") : 0;
  a.tw = d.contains("tw") ? I(d, "tw") : 0; a.seg = d.contains("seg") ? I(d, "seg") : 0;
  a.algo = d.contains("algo") ? I(d, "algo") : 0; a.pd = d.contains("pd") ? I(d, "pd") : 0;
  return a;
}

void chk(hipError_t e, const char* what) { check_hip(e, what); }

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "kdl MI355X (gfx950) HIP kernels and native executor";

  m.def("conv_gemm", [](int mode, int cfg, py::dict d, uintptr_t s) {
    const auto a = conv_args(d);
    py::gil_scoped_release nogil;
    chk(conv_gemm(mode, cfg, a, S(s)), "conv_gemm");
  });
  m.def("conv_gemm_config", [](int cfg) {
    int bm = 0, bn = 0, th = 0;
    if (conv_gemm_config(cfg, &bm, &bn, &th) != 0) throw std::out_of_range("bad conv_gemm config");
    return py::make_tuple(bm, bn, th);
  });
  m.def("conv_gemm_num_configs", &conv_gemm_num_configs);
  // raw async copy (kind: hipMemcpyKind, 1 = H2D, 2 = D2H): the pipelined ingress /
  // egress of bench.py and the serving executor without torch's per-copy bookkeeping
  m.def("memcpy_async", [](uintptr_t dst, uintptr_t src, size_t n, int kind, uintptr_t s) {
    py::gil_scoped_release nogil;
    chk(hipMemcpyAsync((void*)dst, (const void*)src, n, (hipMemcpyKind)kind, S(s)), "memcpy_async");
  });
  m.def("dw3x3", [](py::dict d, uintptr_t s) {
    const auto a = dw_args(d);
    py::gil_scoped_release nogil;
    chk(dw3x3(a, S(s)), "dw3x3");
  });
  m.def("stem_conv", [](py::dict d, uintptr_t s) {
    const auto a = stem_args(d);
    py::gil_scoped_release nogil;
    chk(stem_conv(a, S(s)), "stem_conv");
  });
  m.def("stem_conv3x3", [](int cfg, py::dict d, uintptr_t s) {
    const auto a = stem_conv_args(d);
    py::gil_scoped_release nogil;
    chk(stem_conv3x3(cfg, a, S(s)), "stem_conv3x3");
  });
  m.def("stem_conv3x3_config", [](int cfg) {
    int bm = 0, bn = 0, th = 0;
    if (stem_conv3x3_config(cfg, &bm, &bn, &th) != 0) throw std::out_of_range("bad stem_conv3x3 config");
    return py::make_tuple(bm, bn, th);
  });
  m.def("pool_add", [](py::dict d, uintptr_t s) {
    const auto a = pool_args(d);
    py::gil_scoped_release nogil;
    chk(pool_add(a, S(s)), "pool_add");
  });
  m.def("head_dense", [](py::dict d, uintptr_t s) {
    const auto a = head_args(d);
    py::gil_scoped_release nogil;
    chk(head_dense(a, S(s)), "head_dense");
  });
  m.def("softmax_topk", [](py::dict d, uintptr_t s) {
    const auto a = topk_args(d);
    py::gil_scoped_release nogil;
    chk(softmax_topk(a, S(s)), "softmax_topk");
  });
  m.def("embed_rows", [](py::dict d, uintptr_t s) {
    const auto a = embed_rows_args(d);
    py::gil_scoped_release nogil;
    chk(embed_rows(a, S(s)), "embed_rows");
  });
  m.def("gallery_topk", [](py::dict d, uintptr_t s) {
    const auto a = gallery_topk_args(d);
    py::gil_scoped_release nogil;
    chk(gallery_topk(a, S(s)), "gallery_topk");
  });
  m.def("gallery_topk_workspace", [](int B, int N, int K) { return gallery_topk_workspace(B, N, K); });
  m.def("class_map", [](py::dict d, uintptr_t s) {
    const auto a = class_map_args(d);
    py::gil_scoped_release nogil;
    chk(class_map(a, S(s)), "class_map");
  });
  m.def("attn_rollout", [](py::dict d, uintptr_t s) {
    const auto a = attn_rollout_args(d);
    py::gil_scoped_release nogil;
    chk(attn_rollout(a, S(s)), "attn_rollout");
  });
  m.def("rollout_map", [](py::dict d, uintptr_t s) {
    const auto a = rollout_map_args(d);
    py::gil_scoped_release nogil;
    chk(rollout_map(a, S(s)), "rollout_map");
  });
  // rendered heatmap overlays (kernels/overlay.hip): d = the HeatOverlayArgs fields; h_xb / h_yb are HOST addresses
  m.def("heat_overlay", [](py::dict d, uintptr_t s) {
    const auto a = heat_overlay_args(d);
    py::gil_scoped_release nogil;
    chk(heat_overlay(a, S(s)), "heat_overlay");
  });
  // dominant colours (kernels/palette.hip): d = the PaletteArgs fields; h_xb / h_yb are HOST addresses
  m.def("palette", [](py::dict d, uintptr_t s) {
    const auto a = palette_args(d);
    py::gil_scoped_release nogil;
    chk(palette(a, S(s)), "palette");
  });
  m.def("palette_workspace", [](int B) { return palette_workspace(B); });
  m.attr("PALETTE_MAX_K") = int(kPaletteMaxK);
  m.attr("PALETTE_MAX_T") = int(kPaletteMaxT);
  // garment boxes (kernels/locate.hip): d = the LocateArgs fields; h_xb / h_yb are HOST addresses
  m.def("locate", [](py::dict d, uintptr_t s) {
    const auto a = locate_args(d);
    py::gil_scoped_release nogil;
    chk(locate(a, S(s)), "locate");
  });
  m.def("locate_workspace", [](int B, int S) { return locate_workspace(B, S); });
  m.attr("LOCATE_MAX_K") = int(kLocateMaxK);
  m.attr("LOCATE_LDS_RUNS") = int(kLocateLdsRuns);
  // garment cutouts (kernels/cutout.hip): d = the CutoutArgs fields; h_xb / h_yb are HOST addresses
  m.def("cutout", [](py::dict d, uintptr_t s) {
    const auto a = cutout_args(d);
    py::gil_scoped_release nogil;
    chk(cutout(a, S(s)), "cutout");
  });
  m.def("cutout_workspace", [](int B, int S) { return cutout_workspace(B, S); });
  m.attr("CUTOUT_MAX_ROUNDS") = int(kCutoutMaxRounds);
  m.attr("CUTOUT_MAX_SMOOTH") = int(kCutoutMaxSmooth);
  // baseline JPEG encode (kernels/jpeg_encode.hip): d = the JpegEncodeArgs fields; h_hdr is a HOST address
  m.def("jpeg_encode", [](py::dict d, uintptr_t s) {
    const auto a = jpeg_encode_args(d);
    py::gil_scoped_release nogil;
    chk(jpeg_encode(a, S(s)), "jpeg_encode");
  });
  m.def("jpeg_encode_workspace", [](int B, int H, int W, int sampling, int cap) {
    return jpeg_encode_workspace(B, H, W, sampling, cap);
  });
  m.attr("JPEG_HEADER_BYTES") = int(kJpegHeaderBytes);
  m.attr("JPEG_ENC_MAX_SIDE") = int(kJpegEncMaxSide);
  m.attr("JPEG_ENC_MAX_CAP") = int(kJpegEncMaxCap);
  m.attr("OVERLAY_MAX_S") = int(kOverlayMaxS);
  m.attr("OVERLAY_MAX_TAPS") = int(kOverlayMaxTaps);
  m.attr("ROLLOUT_MAX_T") = int(kRolloutMaxT);
  m.attr("CLASS_MAP_MAX_F") = int(kClassMapMaxF);
  m.attr("CLASS_MAP_MAX_HW") = int(kClassMapMaxHW);
  m.attr("CLASS_MAP_MAX_NC") = int(kClassMapMaxNC);
  m.attr("CLASS_MAP_MAX_H1") = int(kClassMapMaxH1);
  m.attr("GALLERY_MAX_N") = int(kGalleryMaxN);
  m.attr("GALLERY_CHUNK") = int(kGalleryChunk);
  m.attr("EMBED_MAX_F") = int(kEmbedMaxF);
  m.attr("TOPK_MAX_NC") = int(kTopkMaxNC);
  m.attr("TOPK_MAX_K") = int(kTopkMaxK);
  m.def("gap", [](py::dict d, uintptr_t s) {
    const auto a = gap_args(d);
    py::gil_scoped_release nogil;
    chk(gap(a, S(s)), "gap");
  });
  m.def("fc", [](py::dict d, uintptr_t s) {
    const auto a = fc_args(d);
    py::gil_scoped_release nogil;
    chk(fc(a, S(s)), "fc");
  });
  m.def("patchify", [](py::dict d, uintptr_t s) {
    const auto a = patch_args(d);
    py::gil_scoped_release nogil;
    chk(patchify(a, S(s)), "patchify");
  });
  m.def("embed_tokens", [](py::dict d, uintptr_t s) {
    const auto a = embed_args(d);
    py::gil_scoped_release nogil;
    chk(embed_tokens(a, S(s)), "embed_tokens");
  });
  m.def("layernorm", [](py::dict d, uintptr_t s) {
    const auto a = ln_args(d);
    py::gil_scoped_release nogil;
    chk(layernorm(a, S(s)), "layernorm");
  });
  m.def("attention", [](py::dict d, uintptr_t s) {
    const auto a = attn_args(d);
    py::gil_scoped_release nogil;
    chk(attention(a, S(s)), "attention");
  });
  m.def("dwk", [](py::dict d, uintptr_t s) {
    const auto a = dwk_args(d);
    py::gil_scoped_release nogil;
    chk(dwk(a, S(s)), "dwk");
  });
  m.def("dwk_tiles", [](py::dict d) {
    const auto a = dwk_args(d);
    int cg, rb, tw, nt;
    dwk_tiles(a, &cg, &rb, &tw, &nt);
    return py::make_tuple(cg, rb, tw, nt, dwk_seg(a));
  });
  m.def("dwk_plan", [](py::dict d) {
    const auto a = dwk_args(d);
    DwkPlan p{};
    chk(dwk_plan(a, &p), "dwk_plan");
    py::dict r;
    r["algo"] = p.algo; r["cb"] = p.cb; r["rb"] = p.rb; r["tw"] = p.tw; r["seg"] = p.seg; r["pd"] = p.pd;
    r["ntiles"] = p.ntiles; r["lds"] = p.lds;
    return r;
  });
  m.def("squeeze_excite", [](py::dict d, uintptr_t s) {
    const auto a = se_args(d);
    py::gil_scoped_release nogil;
    chk(squeeze_excite(a, S(s)), "squeeze_excite");
  });
  m.def("channel_scale", [](py::dict d, uintptr_t s) {
    const auto a = chs_args(d);
    py::gil_scoped_release nogil;
    chk(channel_scale(a, S(s)), "channel_scale");
  });
  m.def("entry_block", [](int cfg, py::dict d, uintptr_t s) {
    const auto a = eb_args(d);
    py::gil_scoped_release nogil;
    chk(entry_block(cfg, a, S(s)), "entry_block");
  });
  m.def("entry_block_config", [](int cfg) {
    int c0 = 0, c1 = 0, pc = 0, lds = 0;
    if (entry_block_config(cfg, &c0, &c1, &pc, &lds) != 0) throw std::out_of_range("bad entry_block config");
    return py::make_tuple(c0, c1, pc, lds);
  });
  m.def("gemm_f8", [](int cfg, py::dict d, uintptr_t s) {
    const auto a = f8_args(d);
    py::gil_scoped_release nogil;
    chk(gemm_f8(cfg, a, S(s)), "gemm_f8");
  });
  m.def("gemm_f8_config", [](int cfg) {
    int bm = 0, bn = 0, th = 0;
    if (gemm_f8_config(cfg, &bm, &bn, &th) != 0) throw std::out_of_range("bad gemm_f8 config");
    return py::make_tuple(bm, bn, th);
  });
  m.def("fc_mfma", [](py::dict d, uintptr_t s) {
    const auto a = fcm_args(d);
    py::gil_scoped_release nogil;
    chk(fc_mfma(a, S(s)), "fc_mfma");
  });
  m.def("resize_nearest_u8", [](py::dict d, uintptr_t s) {
    const auto a = resize_args(d);
    py::gil_scoped_release nogil;
    chk(resize_nearest_u8(a, S(s)), "resize_nearest_u8");
  });
  // baseline JPEG (kernels/jpeg.hip): d = the JpegArgs fields; h_desc is a HOST address
  m.def("jpeg_idct_u8", [](py::dict d, uintptr_t s) {
    const auto a = jpeg_args(d);
    py::gil_scoped_release nogil;
    chk(jpeg_idct_u8(a, S(s)), "jpeg_idct_u8");
  });
  m.def("jpeg_sample_rgb_u8", [](py::dict d, uintptr_t s) {
    const auto a = jpeg_args(d);
    py::gil_scoped_release nogil;
    chk(jpeg_sample_rgb_u8(a, S(s)), "jpeg_sample_rgb_u8");
  });
  // baseline JPEG entropy decode (kernels/jpeg_huff.hip): d = the JpegHuffArgs fields; h_desc is a HOST address
  m.def("jpeg_huff_decode", [](py::dict d, uintptr_t s) {
    const auto a = jpeg_huff_args(d);
    py::gil_scoped_release nogil;
    chk(jpeg_huff_decode(a, S(s)), "jpeg_huff_decode");
  });
  m.def("jpeg_dc_scan", [](py::dict d, uintptr_t s) {
    const auto a = jpeg_huff_args(d);
    py::gil_scoped_release nogil;
    chk(jpeg_dc_scan(a, S(s)), "jpeg_dc_scan");
  });
  // the same for files with restart intervals; h_stage is the HOST address of the staging's copy
  m.def("jpeg_huff_rst_decode", [](py::dict d, uintptr_t s) {
    const auto a = jpeg_huff_args(d);
    py::gil_scoped_release nogil;
    chk(jpeg_huff_rst_decode(a, S(s)), "jpeg_huff_rst_decode");
  });
  m.def("jpeg_dc_rst_scan", [](py::dict d, uintptr_t s) {
    const auto a = jpeg_huff_args(d);
    py::gil_scoped_release nogil;
    chk(jpeg_dc_rst_scan(a, S(s)), "jpeg_dc_rst_scan");
  });
  m.attr("JPEG_HUFF_SUB_BITS") = int(kJpegHuffSubBits);
  m.attr("JPEG_HUFF_CHUNK") = int(kJpegHuffChunk);
  m.attr("JPEG_HUFF_DESC_BYTES") = int(sizeof(JpegHuffDesc));
  // Pillow's filtered resize (kernels/resample.hip): d = the ResampleArgs fields; h_desc, h_jdesc
  // and the h_xb / h_yb of every descriptor are HOST addresses. kind: 0 raw pixels, 1 JPEG planes
  m.def("resample_h_u8", [](py::dict d, int kind, uintptr_t s) {
    const auto a = resample_args(d);
    py::gil_scoped_release nogil;
    chk(resample_h_u8(a, kind, S(s)), "resample_h_u8");
  });
  m.def("resample_v_u8", [](py::dict d, uintptr_t s) {
    const auto a = resample_args(d);
    py::gil_scoped_release nogil;
    chk(resample_v_u8(a, S(s)), "resample_v_u8");
  });
  m.def("u8_to_bf16_norm", [](uintptr_t x, uintptr_t y, long npix, int ldy, uintptr_t s) {
    py::gil_scoped_release nogil;
    chk(u8_to_bf16_norm(reinterpret_cast<const uint8_t*>(x), reinterpret_cast<uint16_t*>(y), npix, ldy, S(s)),
        "u8_to_bf16_norm");
  });

  // device backend of the native batch executor (kdl._rt.Executor drives it from a C++ thread)
  py::class_<HipExecBackend>(m, "HipExecBackend")
      .def(py::init([](int device, int nslots, size_t item_bytes, int max_batch, int out_cols, uintptr_t copy_stream,
                       bool timing) {
             return new HipExecBackend(device, nslots, item_bytes, max_batch, out_cols, S(copy_stream), timing);
           }),
           py::arg("device"), py::arg("nslots"), py::arg("item_bytes"), py::arg("max_batch"), py::arg("out_cols"),
           py::arg("copy_stream") = 0, py::arg("timing") = true)
      // progs[slot][parity][stage]: Program objects kept alive by the caller
      .def("add_recipe", [](HipExecBackend& be, int bucket, std::vector<uintptr_t> streams, std::vector<int> wait_for,
                            py::list progs, std::vector<uintptr_t> dev_in, std::vector<uintptr_t> dev_out) {
        std::vector<hipStream_t> st;
        for (auto v : streams) st.push_back(S(v));
        std::vector<std::vector<std::vector<const Program*>>> pp;
        for (auto slot : progs) {
          std::vector<std::vector<const Program*>> ps;
          for (auto par : slot.cast<py::list>()) {
            std::vector<const Program*> pk;
            for (auto prog : par.cast<py::list>()) pk.push_back(&prog.cast<const Program&>());
            ps.push_back(pk);
          }
          pp.push_back(ps);
        }
        std::vector<void*> di, dout;
        for (auto v : dev_in) di.push_back(reinterpret_cast<void*>(v));
        for (auto v : dev_out) dout.push_back(reinterpret_cast<void*>(v));
        be.add_recipe(bucket, st, wait_for, pp, di, dout);
      })
      .def("api_ptr", [](const HipExecBackend& be) { return reinterpret_cast<uintptr_t>(be.api()); })
      .def("staging_ptr", [](HipExecBackend& be, int slot) { return reinterpret_cast<uintptr_t>(be.staging(slot)); })
      // direct use without the executor (tests): issue + complete of one slot
      .def("run", [](HipExecBackend& be, int slot, int bucket, int n_real) {
        py::gil_scoped_release nogil;
        const float* out = nullptr;
        kdl_device_times t{};
        if (be.issue(slot, bucket, n_real) != 0 || be.complete(slot, &out, &t) != 0)
          throw std::runtime_error("HipExecBackend: batch failed");
        return std::make_tuple(reinterpret_cast<uintptr_t>(out), t.h2d_ms, t.forward_ms, t.d2h_ms);
      });

  // ---- RCCL data-parallel serving (runtime/comm.h)
  m.def("rccl_unique_id", []() { return py::bytes(rccl_unique_id()); });
  py::class_<RcclComm>(m, "RcclComm")
      .def(py::init([](py::bytes id, int nranks, int rank, int device) {
             const std::string s = id;
             py::gil_scoped_release nogil;       // every rank blocks here until all have joined
             return new RcclComm(s, nranks, rank, device);
           }),
           py::arg("id"), py::arg("nranks"), py::arg("rank"), py::arg("device"))
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("size", &RcclComm::size)
      .def("abort", &RcclComm::abort)
      .def("async_error", &RcclComm::async_error)
      // gather `nbytes` per rank to rank 0 on `stream` (device pointers); no extra stream
      .def("gather", [](RcclComm& c, uintptr_t send, uintptr_t recv, size_t nbytes, uintptr_t stream) {
        if (rccl_gather(c, reinterpret_cast<const void*>(send), reinterpret_cast<void*>(recv), nbytes, S(stream)) != 0)
          throw std::runtime_error("rccl_gather failed");
      });
  py::class_<DpLeader>(m, "DpLeader")
      .def(py::init([](HipExecBackend* local, RcclComm* sc, RcclComm* ga, std::vector<int> buckets, double timeout_s,
                       double ping_s) { return new DpLeader(local, sc, ga, std::move(buckets), timeout_s, ping_s); }),
           py::arg("local"), py::arg("scatter"), py::arg("gather"), py::arg("rank_buckets"), py::arg("timeout_s") = 120.0,
           py::arg("ping_s") = 0.0, py::keep_alive<1, 2>(), py::keep_alive<1, 3>(), py::keep_alive<1, 4>())
      .def("api_ptr", [](const DpLeader& l) { return reinterpret_cast<uintptr_t>(l.api()); })
      .def_property_readonly("world", &DpLeader::world)
      .def_property_readonly("steps", &DpLeader::steps)
      .def_property_readonly("broken", &DpLeader::broken)
      .def("send_ctrl", [](DpLeader& l, int cmd, int version) {
        py::gil_scoped_release nogil;
        return l.send_ctrl(cmd, version);
      })
      .def("ping", [](DpLeader& l) {
        py::gil_scoped_release nogil;
        return l.ping();
      })
      // direct use without the executor (tests / bench): issue + complete of one slot
      .def("run", [](DpLeader& l, int slot, int bucket, int n_real) {
        py::gil_scoped_release nogil;
        const float* out = nullptr;
        kdl_device_times t{};
        if (l.issue(slot, bucket, n_real) != 0 || l.complete(slot, &out, &t) != 0)
          throw std::runtime_error("DpLeader: step failed");
        return reinterpret_cast<uintptr_t>(out);
      });
  py::class_<DpFollower>(m, "DpFollower")
      .def(py::init([](HipExecBackend* local, RcclComm* sc, RcclComm* ga) { return new DpFollower(local, sc, ga); }),
           py::keep_alive<1, 2>(), py::keep_alive<1, 3>(), py::keep_alive<1, 4>())
      .def_property_readonly("steps", &DpFollower::steps)
      // serve until DP_STOP / DP_RELOAD; returns (cmd, version, seq). Raises RuntimeError when rank 0
      // is silent for liveness_s (it pings while idle) or a communicator failed.
      .def("run", [](DpFollower& f, double liveness_s) {
        DpCtrl c{};
        {
          py::gil_scoped_release nogil;
          c = f.run(liveness_s);
        }
        return std::make_tuple(c.cmd, c.version, c.seq);
      }, py::arg("liveness_s") = 30.0);
  // ---- the same protocol over the HIP loopback platform (runtime/dp_hiploop.h): real engines,
  // streams and events on one GPU, ranks as threads of this process, device-to-device transport
  m.def("hiploop_unique_id", []() { return loop::unique_id(); });
  // module_local: kdl._rt registers the same C++ type (loop::Comm) as LoopComm
  py::class_<loop::Comm>(m, "HipLoopComm", py::module_local())
      .def(py::init<const std::string&, int, int>(), py::arg("id"), py::arg("nranks"), py::arg("rank"))
      .def_property_readonly("rank", &loop::Comm::rank)
      .def_property_readonly("size", &loop::Comm::size)
      .def("kill", &loop::Comm::kill)           // this rank stops matching: a dead process
      .def("abort", &loop::Comm::abort)
      .def("error", &loop::Comm::error);
  struct HLLeader {
    std::unique_ptr<HipLoopLocal> local;
    std::unique_ptr<HipLoopDpLeader> lead;
  };
  struct HLFollower {
    std::unique_ptr<HipLoopLocal> local;
    std::unique_ptr<HipLoopDpFollower> f;
  };
  py::class_<HLLeader>(m, "HipLoopDpLeader")
      .def(py::init([](HipExecBackend* be, loop::Comm* sc, loop::Comm* ga, std::vector<int> buckets, double timeout_s,
                       double ping_s) {
             auto h = new HLLeader();
             h->local = std::make_unique<HipLoopLocal>(be);
             h->lead = std::make_unique<HipLoopDpLeader>(h->local.get(), sc, ga, std::move(buckets), timeout_s, ping_s);
             return h;
           }),
           py::arg("local"), py::arg("scatter"), py::arg("gather"), py::arg("rank_buckets"), py::arg("timeout_s") = 120.0,
           py::arg("ping_s") = 0.0, py::keep_alive<1, 2>(), py::keep_alive<1, 3>(), py::keep_alive<1, 4>())
      .def("api_ptr", [](const HLLeader& l) { return reinterpret_cast<uintptr_t>(l.lead->api()); })
      .def_property_readonly("world", [](const HLLeader& l) { return l.lead->world(); })
      .def_property_readonly("steps", [](const HLLeader& l) { return l.lead->steps(); })
      .def_property_readonly("broken", [](const HLLeader& l) { return l.lead->broken(); })
      .def("send_ctrl", [](HLLeader& l, int cmd, int version) {
        py::gil_scoped_release nogil;
        return l.lead->send_ctrl(cmd, version);
      })
      .def("ping", [](HLLeader& l) {
        py::gil_scoped_release nogil;
        return l.lead->ping();
      });
  py::class_<HLFollower>(m, "HipLoopDpFollower")
      .def(py::init([](HipExecBackend* be, loop::Comm* sc, loop::Comm* ga) {
             auto h = new HLFollower();
             h->local = std::make_unique<HipLoopLocal>(be);
             h->f = std::make_unique<HipLoopDpFollower>(h->local.get(), sc, ga);
             return h;
           }),
           py::keep_alive<1, 2>(), py::keep_alive<1, 3>(), py::keep_alive<1, 4>())
      .def_property_readonly("steps", [](const HLFollower& f) { return f.f->steps(); })
      .def("run", [](HLFollower& f, double liveness_s) {
        DpCtrl c{};
        {
          py::gil_scoped_release nogil;
          c = f.f->run(liveness_s);
        }
        return std::make_tuple(c.cmd, c.version, c.seq);
      }, py::arg("liveness_s") = 30.0);
  m.attr("DP_STOP") = int(DP_STOP);
  m.attr("DP_BATCH") = int(DP_BATCH);
  m.attr("DP_RELOAD") = int(DP_RELOAD);
  m.attr("DP_PING") = int(DP_PING);

  py::class_<Program>(m, "Program")
      .def(py::init<>())
      .def("add_conv_gemm", [](Program& p, const std::string& name, int mode, int cfg, py::dict d) {
        Op op; op.kind = OP_CONV_GEMM; op.name = name; op.mode = mode; op.cfg = cfg; op.g = conv_args(d);
        p.add(op);
      })
      .def("add_stem", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_STEM; op.name = name; op.st = stem_args(d); p.add(op);
      })
      .def("add_stem_conv", [](Program& p, const std::string& name, int cfg, py::dict d) {
        Op op; op.kind = OP_STEM_CONV; op.name = name; op.cfg = cfg; op.sc = stem_conv_args(d); p.add(op);
      })
      .def("add_pool_add", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_POOL_ADD; op.name = name; op.pa = pool_args(d); p.add(op);
      })
      .def("add_head", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_HEAD; op.name = name; op.hd = head_args(d); p.add(op);
      })
      .def("add_softmax_topk", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_SOFTMAX_TOPK; op.name = name; op.tk = topk_args(d); p.add(op);
      })
      .def("add_embed_rows", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_EMBED_ROWS; op.name = name; op.er = embed_rows_args(d); p.add(op);
      })
      .def("add_class_map", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_CLASS_MAP; op.name = name; op.cm = class_map_args(d); p.add(op);
      })
      .def("add_attn_rollout", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_ATTN_ROLLOUT; op.name = name; op.ar = attn_rollout_args(d); p.add(op);
      })
      .def("add_rollout_map", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_ROLLOUT_MAP; op.name = name; op.rm = rollout_map_args(d); p.add(op);
      })
      .def("add_heat_overlay", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_HEAT_OVERLAY; op.name = name; op.ho = heat_overlay_args(d); p.add(op);
      })
      .def("add_palette", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_PALETTE; op.name = name; op.pal = palette_args(d); p.add(op);
      })
      .def("add_locate", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_LOCATE; op.name = name; op.loc = locate_args(d); p.add(op);
      })
      .def("add_cutout", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_CUTOUT; op.name = name; op.cut = cutout_args(d); p.add(op);
      })
      .def("add_jpeg_encode", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_JPEG_ENCODE; op.name = name; op.je = jpeg_encode_args(d); p.add(op);
      })
      .def("add_gallery_topk", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_GALLERY_TOPK; op.name = name; op.gt = gallery_topk_args(d); p.add(op);
      })
      .def("add_gap", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_GAP; op.name = name; op.gp = gap_args(d); p.add(op);
      })
      .def("add_fc", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_FC; op.name = name; op.fc = fc_args(d); p.add(op);
      })
      .def("add_patchify", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_PATCHIFY; op.name = name; op.pt = patch_args(d); p.add(op);
      })
      .def("add_embed", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_EMBED; op.name = name; op.em = embed_args(d); p.add(op);
      })
      .def("add_layernorm", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_LN; op.name = name; op.ln = ln_args(d); p.add(op);
      })
      .def("add_attention", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_ATTN; op.name = name; op.at = attn_args(d); p.add(op);
      })
      .def("add_dwk", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_DWK; op.name = name; op.dk = dwk_args(d); p.add(op);
      })
      .def("add_se", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_SE; op.name = name; op.se = se_args(d); p.add(op);
      })
      .def("add_chscale", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_CHSCALE; op.name = name; op.cs = chs_args(d); p.add(op);
      })
      .def("add_entry_block", [](Program& p, const std::string& name, int cfg, py::dict d) {
        Op op; op.kind = OP_ENTRY_BLOCK; op.name = name; op.cfg = cfg; op.eb = eb_args(d); p.add(op);
      })
      .def("add_gemm_f8", [](Program& p, const std::string& name, int cfg, py::dict d) {
        Op op; op.kind = OP_GEMM_F8; op.name = name; op.cfg = cfg; op.f8 = f8_args(d); p.add(op);
      })
      .def("add_fc_mfma", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_FC_MFMA; op.name = name; op.fcm = fcm_args(d); p.add(op);
      })
      .def("add_resize", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_RESIZE; op.name = name; op.rs = resize_args(d); p.add(op);
      })
      .def("add_dw", [](Program& p, const std::string& name, py::dict d) {
        Op op; op.kind = OP_DW; op.name = name; op.dw = dw_args(d); p.add(op);
      })
      .def("add_memset", [](Program& p, const std::string& name, uintptr_t ptr, size_t bytes) {
        Op op; op.kind = OP_MEMSET; op.name = name; op.mem_ptr = reinterpret_cast<void*>(ptr);
        op.mem_bytes = bytes; p.add(op);
      })
      .def("set_cfg", [](Program& p, size_t i, int cfg) { p.mutable_op(i).cfg = cfg; })
      .def("cfg", [](const Program& p, size_t i) { return p.op(i).cfg; })
      .def("op_names", [](const Program& p) {
        std::vector<std::string> v;
        for (size_t i = 0; i < p.size(); ++i) v.push_back(p.op(i).name);
        return v;
      })
      .def("__len__", &Program::size)
      .def("run", [](const Program& p, uintptr_t s) { py::gil_scoped_release nogil; p.run(S(s)); })
      .def("capture", [](Program& p, uintptr_t s) { py::gil_scoped_release nogil; p.capture(S(s)); })
      .def("launch", [](const Program& p, uintptr_t s) { py::gil_scoped_release nogil; p.launch(S(s)); })
      .def("reset", &Program::reset)
      .def_property_readonly("captured", &Program::captured)
      .def("profile", [](const Program& p, uintptr_t s, int iters) {
        py::gil_scoped_release nogil;
        return p.profile(S(s), iters);
      });
}
