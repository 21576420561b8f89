// gdm_parts.h -- the one scheme by which a kernel family compiles as one unit
// per degree.  The kernels of one degree can take minutes to compile, so such a
// source is compiled once per degree, side by side: -DGDM_PART=<p> selects the
// unit of degree p and, where the family has degree-independent code,
// -DGDM_PART=0 the unit that holds it (csrc/Makefile: gdm_family).  A unit of
// degree p defines its entry points as GDM_PART_NAME(stem); the callers declare
// stem1 ... stem9 from one signature and pick one by the run-time degree.
#pragma once

// The degrees with a unit.  X is called as X(p, args...): define it with a
// trailing `...` even where it takes no further argument.
#define GDM_FOR_EACH_DEGREE(X, ...) \
  X(1, __VA_ARGS__) X(3, __VA_ARGS__) X(5, __VA_ARGS__) X(7, __VA_ARGS__) X(9, __VA_ARGS__)
// the degrees of the single-sweep mass solve (gdm_mass.hip)
#define GDM_FOR_EACH_MASS3_DEGREE(X, ...) X(3, __VA_ARGS__) X(5, __VA_ARGS__) X(7, __VA_ARGS__)

#define GDM_PARTS_CAT_(a, b) a##b
#define GDM_PARTS_CAT(a, b) GDM_PARTS_CAT_(a, b)
// stem<GDM_PART>, in a unit compiled with -DGDM_PART=<p>
#define GDM_PART_NAME(stem) GDM_PARTS_CAT(stem, GDM_PART)

// hipError_t stem<p>(signature...); for every degree of LIST
#define GDM_PARTS_DECLARE_(p, stem, ...) hipError_t stem##p(__VA_ARGS__);
#define GDM_PARTS_DECLARE_IN(LIST, stem, ...) LIST(GDM_PARTS_DECLARE_, stem, __VA_ARGS__)
#define GDM_PARTS_DECLARE(stem, ...) GDM_PARTS_DECLARE_IN(GDM_FOR_EACH_DEGREE, stem, __VA_ARGS__)

// return stem<deg>(args...); a degree that is not in LIST returns dflt
#define GDM_PARTS_CASE_(p, stem, ...) \
  case p: return stem##p(__VA_ARGS__);
#define GDM_PARTS_SWITCH_IN(LIST, deg, dflt, stem, ...) \
  switch (deg) {                                        \
    LIST(GDM_PARTS_CASE_, stem, __VA_ARGS__)            \
    default: return dflt;                               \
  }
#define GDM_PARTS_SWITCH(deg, dflt, stem, ...) GDM_PARTS_SWITCH_IN(GDM_FOR_EACH_DEGREE, deg, dflt, stem, __VA_ARGS__)
