// Limits shared by the GroupNorm kernels (groupnorm.hip) and their torch
// wrappers (bindings.cpp).
#pragma once

// Largest ch/G (channels per normalisation group): the backward kernels
// keep per-channel dgamma/dbeta partials in LDS arrays of this length.
#define MAX_CG 128
