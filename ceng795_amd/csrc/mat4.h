// The reference's fp32 4x4 matrices (HW3/src/Matrix4x4.cpp, PPM/src/Matrix4x4.cpp: the same code),
// shared by the photon-mapping scene loader (ppm_scene.cpp) and the instanced ray-tracing scenes
// (instances.cpp).  Host only; every file that includes it compiles with contraction off, so each
// product and sum rounds once, in the order written there.
#ifndef CENG795_MAT4_H_
#define CENG795_MAT4_H_

#include <cstring>

namespace rt {

struct Mat4 {
  float a[4][4];
  static Mat4 zero() {
    Mat4 m;
    std::memset(m.a, 0, sizeof m.a);
    return m;
  }
  static Mat4 identity() {
    Mat4 m = zero();
    for (int i = 0; i < 4; i++) m.a[i][i] = 1.0f;
    return m;
  }
  Mat4 operator*(const Mat4& r) const {  // result[i][j] += a[i][k] * r[k][j], k ascending
    Mat4 o = zero();
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++)
        for (int k = 0; k < 4; k++) o.a[i][j] += a[i][k] * r.a[k][j];
    return o;
  }
  Mat4 transposed() const {
    Mat4 t;
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) t.a[i][j] = a[j][i];
    return t;
  }
  // multiply(v, false): a point.  r and v may not alias.
  void point(const float v[3], float r[3]) const {
    for (int i = 0; i < 3; i++) {
      r[i] = a[i][3];
      r[i] += a[i][0] * v[0];
      r[i] += a[i][1] * v[1];
      r[i] += a[i][2] * v[2];
    }
  }
  // multiply(v, true): a vector (starts from 0, so a -0 sum comes out +0 as there)
  void vector(const float v[3], float r[3]) const {
    for (int i = 0; i < 3; i++) {
      r[i] = 0;
      r[i] += a[i][0] * v[0];
      r[i] += a[i][1] * v[1];
      r[i] += a[i][2] * v[2];
    }
  }
  bool identity_p() const {
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++)
        if (a[i][j] != (i == j ? 1.0f : 0.0f)) return false;
    return true;
  }
  // Matrix4x4::invert_matrix: cofactors as written there, det = 1/det, inv * det.
  bool inverse(Mat4& out) const {
    float m[16], c[16];
    for (int k = 0; k < 16; k++) m[k] = a[k / 4][k % 4];
    c[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] +
           m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    c[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] -
           m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    c[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] +
           m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    c[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] -
            m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    c[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] -
           m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    c[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] +
           m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    c[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] -
           m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    c[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] +
            m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    c[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] +
           m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    c[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] -
           m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    c[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] +
            m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    c[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] -
            m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    c[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] -
           m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    c[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] +
           m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    c[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] -
            m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    c[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] +
            m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    float det = m[0] * c[0] + m[1] * c[4] + m[2] * c[8] + m[3] * c[12];
    if (det == 0.0f) return false;
    det = 1.0f / det;
    for (int k = 0; k < 16; k++) out.a[k / 4][k % 4] = c[k] * det;
    return true;
  }
};

}  // namespace rt

#endif
