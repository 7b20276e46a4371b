// One layer of the Llama decoders' K / V cache: ONE owner of its layout, a pure function of (mode, rows, n_kv, head_dim, P).
// The engine's cache is n_layers such layers back to back; production (llama_kv_layer, ensure_llama_gen) and the debug entries
// address it through this function and hold no layout arithmetic of their own.  All figures are BYTES from the layer's start.
//   mode 0 (fp16 cache) and 2 (an FP8-cache engine's dequantised fp16 values):   K [rows][n_kv][P][head_dim] fp16 | V
//   mode 1 (FP8 bytes, head_dim 128: llama_kernels_kv8.h):   K bytes [rows][n_kv][P][head_dim] | V bytes |
//                                                            K exponents [rows][n_kv][pe] int8 | V exponents,  pe = P rounded up to 32
// Every region is a multiple of 32 bytes long (head_dim a multiple of 16; pe of 32), so in a 32-byte aligned block every region of
// every layer starts 32-byte aligned - the step kernel reads a wave's 32 exponents as two aligned 16-byte loads.
// Plain C++17, no HIP: a CPU program includes this header too (tests/test_kv_layout_host.py).
#pragma once
#include <cstddef>

struct KvLayerLayout {
  size_t k = 0, v = 0, ke = 0, ve = 0;                     // the regions' offsets (ke = ve = 0 outside mode 1: not there)
  size_t bytes = 0;                                        // the layer
  int pe = 0;                                              // an exponent row's length (0 outside mode 1)
};
constexpr KvLayerLayout kv_layer_layout(int mode, int rows, int n_kv, int head_dim, int P) {
  KvLayerLayout L;
  const size_t heads = (size_t)rows * n_kv, plane = heads * P * head_dim * (mode == 1 ? 1 : 2);
  L.v = plane;
  L.bytes = 2 * plane;
  if (mode != 1) return L;
  L.pe = (P + 31) & ~31;
  L.ke = 2 * plane;
  L.ve = L.ke + heads * L.pe;
  L.bytes = L.ve + heads * L.pe;
  return L;
}
