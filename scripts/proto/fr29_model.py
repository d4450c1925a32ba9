#!/usr/bin/env python3
import os, sys; sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import fr29_model; print("fr29 model ok: %d products, %d butterflies" % fr29_model.sampled_checks())          # the model and its tests: tests/fr29_model.py, tests/test_fr29_model.py
