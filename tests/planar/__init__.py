"""The CPU restatement of the planar (2D) clustering main: test infrastructure (planar_ref.h)."""
