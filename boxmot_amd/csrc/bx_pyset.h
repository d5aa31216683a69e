// bx_pyset.h — iteration order of a CPython set of small non-negative ints, on host and device.
//
// StrongSort's occlusion handling averages the centres of a track's occluders in the order a
// Python `set` of their ids iterates (utils/occlusion_handler.py:268-305), and that order decides
// the bits of the sum.  CPython (3.10, Objects/setobject.c) keeps a set of ints as an open table:
//   * hash(i) = i; the first slot is i & mask, then 9 linear probes when they fit below the
//     table's end, then `perturb >>= 5; i = (i * 5 + 1 + perturb) & mask`;
//   * after an insertion with fill * 5 >= mask * 3 the table is rebuilt at the first power of two
//     above 4 * fill (entries re-inserted in table order, the same probing without the compare);
//   * iteration walks the table from slot 0.
// The table here stores 1 + (index into `adds`) so that key 0 and an empty slot stay apart and a
// caller gets back positions, not values.
#ifndef BX_PYSET_H
#define BX_PYSET_H

#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BX_PYSET_FN __host__ __device__ inline
#else
#define BX_PYSET_FN inline
#endif

// Slots of the table after n distinct keys were added (8, 32, 128, 512, 2048, ...).
BX_PYSET_FN int bx_pyset_cap(int n) {
  long mask = 7;
  for (long fill = 1; fill <= n; fill++)
    if (fill * 5 >= mask * 3) {
      long nsz = 8;
      while (nsz <= fill * 4) nsz <<= 1;
      mask = nsz - 1;
    }
  return (int)(mask + 1);
}

// Adds adds[0..n) in order and writes to out the positions (into adds) of the distinct keys in the
// set's iteration order; returns their number.  ta and tb: scratch tables of bx_pyset_cap(n) ints
// each (the rebuild goes from one to the other).  Serial: one thread.
template <class K>
BX_PYSET_FN int bx_pyset_order(const K* adds, int n, int* ta, int* tb, int* out) {
  int* tab = ta;
  int* other = tb;
  size_t mask = 7;
  long fill = 0;
  for (int q = 0; q < 8; q++) tab[q] = 0;
  for (int a = 0; a < n; a++) {
    const K key = adds[a];
    size_t perturb = (size_t)key, i = (size_t)key & mask;
    long at = -1;
    bool dup = false;
    for (;;) {  // set_add_entry
      size_t e = i;
      int probes = (i + 9 <= mask) ? 9 : 0;
      do {
        const int v = tab[e];
        if (v == 0) {
          at = (long)e;
          break;
        }
        if (adds[v - 1] == key) {
          dup = true;
          break;
        }
        e++;
      } while (probes--);
      if (at >= 0 || dup) break;
      perturb >>= 5;
      i = (i * 5 + 1 + perturb) & mask;
    }
    if (dup) continue;
    tab[at] = a + 1;
    fill++;
    if ((size_t)fill * 5 < mask * 3) continue;
    size_t nsz = 8;  // set_table_resize(used * 4) + set_insert_clean
    while (nsz <= (size_t)fill * 4) nsz <<= 1;
    const size_t nmask = nsz - 1;
    for (size_t q = 0; q < nsz; q++) other[q] = 0;
    for (size_t q = 0; q <= mask; q++) {
      const int v = tab[q];
      if (!v) continue;
      size_t pp = (size_t)adds[v - 1], j = pp & nmask;
      for (;;) {
        size_t e = j;
        int probes = (j + 9 <= nmask) ? 9 : 0;
        bool done = false;
        do {
          if (other[e] == 0) {
            other[e] = v;
            done = true;
            break;
          }
          e++;
        } while (probes--);
        if (done) break;
        pp >>= 5;
        j = (j * 5 + 1 + pp) & nmask;
      }
    }
    int* sw = tab;
    tab = other;
    other = sw;
    mask = nmask;
  }
  int m = 0;
  for (size_t q = 0; q <= mask; q++)
    if (tab[q]) out[m++] = tab[q] - 1;
  return m;
}

#endif  // BX_PYSET_H
