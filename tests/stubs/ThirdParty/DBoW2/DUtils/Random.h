// Declarations-only stand-in for DBoW2's DUtils/Random.h (tools/check_integration_syntax.py): what integration/CubemapHipBridge.cpp names of it.
#ifndef STUB_DUTILS_RANDOM_H
#define STUB_DUTILS_RANDOM_H
namespace DUtils {
class Random {
 public:
  static int RandomInt(int min, int max);
};
}
#endif
