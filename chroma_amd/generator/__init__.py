"""Photon generators that need no GPU (reference package: chroma/generator; its GEANT4 generator is out of scope).
``steps``: photons from the step points of charged particles, over the library's host loops."""
from chroma_amd.generator.steps import (LightSource, Segments, segments_from_vertices, count_photons, generate_photons,
                                        PARTICLES)
