"""The reference's preprocessing tools that the package can reproduce itself."""
