// Test driver (tests/test_qat_truth_cpu.py): float32 values on stdin -> FakeQuantizer(argv[1]).Quantize
// of each on stdout, through the reference's own header where its sources are present.  Compiled at
// test time; no binary is committed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "monolith/native_training/runtime/hash_table/compressor/fake_quantizer.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const monolith::hash_table::FakeQuantizer q(static_cast<float>(atof(argv[1])));
  float f;
  while (fread(&f, sizeof(f), 1, stdin) == 1) {
    const float o = q.Quantize(f);
    fwrite(&o, sizeof(o), 1, stdout);
  }
  return 0;
}
