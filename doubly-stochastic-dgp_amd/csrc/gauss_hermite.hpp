// The 20-point Gauss–Hermite rule of the MultiClass likelihood (multiclass.hip, classification.hip): one table, filled one way.  Each
// translation unit keeps its own __constant__ copy (a device symbol is not shared across objects without relocatable device code).
#pragma once

#define GH20_H 20

// numpy.polynomial.hermite.hermgauss(20): nodes x, weights w / sqrt(pi); symmetric, listed once
static inline void gh20_nodes(double x[GH20_H], double w[GH20_H]) {
  static const double xpos[10] = {0.2453407083009012499, 0.7374737285453943587, 1.2340762153953230079, 1.7385377121165862068,
                                  2.2549740020892756723, 2.7888060584281304806, 3.3478545673832163269, 3.9447640401156252104,
                                  4.6036824495507442731, 5.3874808900112328620};
  static const double wpos[10] = {4.6224366960061008965e-1, 2.8667550536283412972e-1, 1.0901720602002331250e-1,
                                  2.4810520887463643070e-2, 3.2437733422378566463e-3, 2.2833863601635308670e-4,
                                  7.8025564785320636941e-6, 1.0860693707692815356e-7, 4.3993409922731805536e-10,
                                  2.2293936455341516100e-13};
  const double isp = 0.56418958354775628695;   // 1/sqrt(pi)
  for (int i = 0; i < 10; ++i) {
    x[10 + i] = xpos[i];  w[10 + i] = wpos[i] * isp;
    x[9 - i] = -xpos[i];  w[9 - i] = wpos[i] * isp;
  }
}
